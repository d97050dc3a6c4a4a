"""solver_args newton_first at the plugin level (interfaces/newton_first.py): a warm-started call takes Newton steps first, accepts what
passes the solver's own termination test and solves the rest by the ordinary kernels.

Recipe of every case (the one the feature was specified with): the warm start is the oracle's eps = 1e-6 point of the UNPERTURBED data, given as an explicit
triple; the call's data is that data with every entry of A, b, c multiplied by 1 + rel N(0, 1) (newton_first_kit.perturb, default_rng(seed + 100)); the box QP
moves b, c and one scalar on P per instance (default_rng(102)).  References: the oracle at eps = 1e-10 on the perturbed data under the project's eps = 1e-8
parity gate 1e-6 (1 + |.|_inf); the numpy termination test; oracle.adjoint_batch under the 1e-5 relative gate; ConeEngine.refine + ConeEngine.solve run by the
test for bit equality of the fallback instances.  Fallback budgets are the specification's: at most 1/8 of the small shape (the dense reference leaves 3 of 64), at
most 2 of 48 of the metric shape (the reference leaves none)."""
import warnings

import numpy as np
import pytest
import torch

from cvxpylayers_amd import problems as P
from newton_first_kit import METRIC, SMALL, perturb, termination_test
from oracle import oracle
from test_quad_objective import _p_values

_CACHE = {}


def _plugin():
    from cvxpylayers_amd.interfaces import mi355_if
    return mi355_if


def _shape(key, rel, planted=False):
    """(tpl, cones, data of the call, warm triple (numpy), reference at eps = 1e-10 on the call's data), computed once"""
    ck = (key, rel, planted)
    if ck not in _CACHE:
        n, cones, B, seed = {"small": SMALL, "metric": METRIC}[key]
        A0, b0, c0 = P.generate(n, cones, B, seed=seed)
        A, b, c = perturb(A0, b0, c0, rel, seed)
        if planted:          # a duplicated equality row, in the warm start's data and in the call's: the elimination flags these instances
            for M, v in ((A0, b0), (A, b)):
                M[PLANT_DUP, 1, :] = M[PLANT_DUP, 0, :]; v[PLANT_DUP, 1] = v[PLANT_DUP, 0]
        w = oracle.solve_batch(A0, b0, c0, cones, eps=1e-6)
        ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=400000) if (rel < 1 and not planted) else None
        _CACHE[ck] = (P.dense_template(n, cones), cones, (A, b, c), (w["x"], w["y"], w["s"]), ref)
    return _CACHE[ck]


PLANT_DUP = [3, 10, 20, 33]
PLANT_NAN = [5, 40]


def _call(tpl, cones, data, warm, args, ctx=None, needs_grad=False):
    m = _plugin()
    dev = torch.device("cuda", 0)
    ctx = ctx if ctx is not None else m.MI355_ctx(None, tpl.problem_data_index, cones)
    A_eval, q_eval = tpl.values_from_dense(*data)
    A_t, q_t = torch.from_numpy(A_eval).to(dev), torch.from_numpy(q_eval).to(dev)
    if needs_grad:
        A_t.requires_grad_(); q_t.requires_grad_()
    w = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in warm) if warm is not None else None
    primal, dual, info, _ = m._CvxpyLayer.apply(None, q_t, A_t, ctx, dict(args), needs_grad, w)
    eng = ctx.engine(dev)
    return dict(x=primal, y=dual, s=eng._last_solution[2], info=info, ctx=ctx, eng=eng, A_t=A_t, q_t=q_t, warm=w)


def _np(t):
    return t.detach().cpu().numpy()


def _parity(r, ref):
    for k in ("x", "y"):
        err = np.abs(_np(r[k]) - ref[k]).max(1); gate = 1e-6 * (1 + np.abs(ref[k]).max(1))
        print(f"    max |{k} - oracle| / gate = {(err / gate).max():.3e}")
        assert (err <= gate).all(), (k, err.max())


def _accepted_pass_numpy(r, data, eps):
    nf = r["info"]["newton_first"]
    acc = _np(nf["accepted"])
    t = termination_test(*data, _np(r["x"]), _np(r["y"]), _np(r["s"]), eps, eps)
    assert (_np(r["info"]["iters"])[acc] == 0).all() and (_np(r["info"]["status"])[acc] == 1).all()
    # (the kernel's own decision, re-made in numpy at the returned point; a residual within rounding of its threshold may differ, by 1e-12 (1 + sum |terms|))
    slack = 1e-12 * (1 + t["terms"])
    assert ((t["resid"] <= t["thr"] + slack) & t["finite"][:, None])[acc].all()
    np.testing.assert_allclose(_np(r["info"]["resid"])[acc], t["resid"][acc], rtol=0, atol=float(slack.max()))
    assert nf["n_accepted"] == int(acc.sum()) and nf["n_fallback"] == int((~acc).sum()) and nf["path"] == "ns"


@pytest.mark.gpu
def test_small_shape_tracks_a_small_change_by_newton_steps():
    tpl, cones, data, warm, ref = _shape("small", 1e-3)
    r = _call(tpl, cones, data, warm, {"eps": 1e-8, "newton_first": 3})
    nf = r["info"]["newton_first"]
    print(f"small rel 1e-3 eps 1e-8 k=3: accepted {nf['n_accepted']}, fallback {nf['n_fallback']}, fallback iters {_np(r['info']['iters'])[~_np(nf['accepted'])]}")
    assert (_np(r["info"]["status"]) == 1).all()
    _parity(r, ref)
    _accepted_pass_numpy(r, data, 1e-8)
    assert nf["steps"] == 3 and nf["refine"]["path"] == "ns"
    assert nf["n_fallback"] <= SMALL[2] // 8


@pytest.mark.gpu
def test_metric_shape_falls_back_on_at_most_two_instances_and_its_gradients_match_the_oracle():
    tpl, cones, data, warm, ref = _shape("metric", 1e-3)
    r = _call(tpl, cones, data, warm, {"eps": 1e-8, "newton_first": 3}, needs_grad=True)
    nf = r["info"]["newton_first"]
    print(f"metric rel 1e-3 eps 1e-8 k=3: accepted {nf['n_accepted']}, fallback {nf['n_fallback']}")
    assert (_np(r["info"]["status"]) == 1).all()
    _parity(r, ref)
    _accepted_pass_numpy(r, data, 1e-8)
    assert nf["n_fallback"] <= 2
    r["x"].sum().backward()
    torch.cuda.synchronize()
    g = oracle.adjoint_batch(*data, cones, ref["x"], ref["y"], ref["s"], np.ones_like(ref["x"]), np.zeros_like(ref["y"]), mode="dense")
    dA, db, dc = tpl.dense_from_values(_np(r["A_t"].grad), _np(r["q_t"].grad))
    acc = _np(nf["accepted"])
    for name, got, want in (("dc", dc, g["dc"]), ("db", db, g["db"]), ("dA", dA, g["dA"])):
        err = np.abs(got - want)[acc].max() / (1 + np.abs(want)[acc].max())
        print(f"    {name}: relative error at the accepted instances {err:.3e}")
        assert err < 1e-5, (name, err)


@pytest.mark.gpu
def test_planted_fallbacks_are_solved_by_the_ordinary_kernels_from_the_refined_point():
    m = _plugin()
    tpl, cones, data, warm, ref = _shape("small", 1e-3, planted=True)
    warm = tuple(t.copy() for t in warm)
    warm[0][PLANT_NAN[0], 2] = np.nan; warm[1][PLANT_NAN[1], 4] = np.nan
    args = {"eps": 1e-8, "newton_first": 3}
    r = _call(tpl, cones, data, warm, args)
    nf, acc = r["info"]["newton_first"], _np(r["info"]["newton_first"]["accepted"])
    assert not acc[PLANT_DUP + PLANT_NAN].any() and (_np(r["info"]["status"]) == 1).all()
    assert (_np(nf["refine"]["status"])[PLANT_DUP] & 4).all(), "the elimination flags a duplicated equality row"
    assert nf["n_fallback"] <= 6 + SMALL[2] // 8
    # the same steps and the same sub-batch solve, run by hand on a second engine
    eng = m.MI355_ctx(None, tpl.problem_data_index, cones).engine(torch.device("cuda", 0))
    A_bm = r["A_t"].detach().t().contiguous(); q_t = r["q_t"].detach()
    x, y, s, _ = eng.refine(A_bm, q_t, *(t.clone() for t in r["warm"]), 3)
    idx = torch.from_numpy(np.nonzero(~acc)[0]).to(A_bm.device)
    sx, sy, ss, siters, sstatus, _ = eng.solve(A_bm[idx].contiguous(), q_t[:, idx].contiguous(), m.make_settings(args), warm=(x[idx], y[idx], s[idx]))
    torch.cuda.synchronize()
    for got, want in ((r["x"][idx], sx), (r["y"][idx], sy), (r["s"][idx], ss), (r["info"]["iters"][idx], siters)):
        np.testing.assert_array_equal(_np(got), _np(want))
    # and the accepted ones are the refined points, bit for bit
    ai = torch.from_numpy(np.nonzero(acc)[0]).to(A_bm.device)
    np.testing.assert_array_equal(_np(r["x"][ai]), _np(x[ai])); np.testing.assert_array_equal(_np(r["y"][ai]), _np(y[ai]))


def _box_qp(rel, B=32):
    nx = 10
    A0, b0, c0, P0, pst, _ = P.native_box_qp_batch(nx, B, seed=2)
    cones = {"z": 0, "l": 2 * nx, "q": []}
    A = np.broadcast_to(A0, (B,) + A0.shape).copy(); Pm0 = np.broadcast_to(P0, (B, nx, nx)).copy()
    rng = np.random.default_rng(102)
    b = b0 * (1 + rel * rng.standard_normal(b0.shape)); c = c0 * (1 + rel * rng.standard_normal(c0.shape)); Pm = Pm0 * (1 + rel * rng.standard_normal((B, 1, 1)))
    w = oracle.solve_batch(A, b0, c0, cones, P=Pm0, eps=1e-6)
    return P.dense_template(nx, cones, pattern=(A0 != 0)), cones, pst, (A, b, c), Pm, (w["x"], w["y"], w["s"])


@pytest.mark.gpu
def test_an_all_accepted_call_launches_no_forward_kernel():
    m = _plugin()
    dev = torch.device("cuda", 0)
    tpl, cones, pst, data, Pm, warm = _box_qp(1e-3)
    ctx = m.MI355_ctx(pst, tpl.problem_data_index, cones)
    eng = ctx.engine(dev)
    assert eng.qp_native
    A_eval, q_eval = tpl.values_from_dense(*data)
    P_eval = torch.from_numpy(np.ascontiguousarray(_p_values(Pm, pst).T)).to(dev)
    w = tuple(torch.from_numpy(t).to(dev) for t in warm)
    eng.set_profiling(True); eng.reset_profile()
    try:
        primal, dual, info, _ = m._CvxpyLayer.apply(P_eval, torch.from_numpy(q_eval).to(dev), torch.from_numpy(A_eval).to(dev), ctx, {"eps": 1e-8, "newton_first": 2}, False, w)
        torch.cuda.synchronize()
        fwd_launches, streaming = eng.profile(0)[1], eng.profile(2)[1]
    finally:
        eng.set_profiling(0); eng.reset_profile()
    nf = info["newton_first"]
    print(f"box QP rel 1e-3 eps 1e-8 k=2: accepted {nf['n_accepted']} of {len(warm[0])}; forward launches {fwd_launches}, class-2 brackets {streaming}")
    assert nf["n_fallback"] == 0 and bool(nf["accepted"].all()) and fwd_launches == 0 and streaming >= 1
    assert (_np(info["iters"]) == 0).all() and (_np(info["status"]) == 1).all()
    ref = oracle.solve_batch(*data, cones, P=Pm, eps=1e-10, max_iters=400000)
    _parity(dict(x=primal, y=dual), ref)
    t = termination_test(*data, _np(primal), _np(dual), _np(eng._last_solution[2]), 1e-8, 1e-8, Pm=Pm)
    assert ((t["resid"] <= t["thr"] + 1e-12 * (1 + t["terms"])) & t["finite"][:, None]).all()


@pytest.mark.gpu
def test_a_call_with_nothing_accepted_equals_the_ordinary_call_from_the_refined_point():
    m = _plugin()
    tpl, cones, data, warm, _ = _shape("small", 10.0)
    args = {"eps": 1e-4, "max_iters": 2000, "raise_on_error": False}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = _call(tpl, cones, data, warm, {**args, "newton_first": 2})
        nf = r["info"]["newton_first"]
        assert nf["n_accepted"] == 0 and nf["n_fallback"] == SMALL[2]
        eng = m.MI355_ctx(None, tpl.problem_data_index, cones).engine(torch.device("cuda", 0))
        x, y, s, _ = eng.refine(r["A_t"].t().contiguous(), r["q_t"], *(t.clone() for t in r["warm"]), 2)
        o = _call(tpl, cones, data, tuple(_np(t) for t in (x, y, s)), {**args, "newton_first": 0})
    for k in ("x", "y", "s"):
        np.testing.assert_array_equal(_np(r[k]), _np(o[k]))
    for k in ("iters", "status", "resid"):
        np.testing.assert_array_equal(_np(r["info"][k]), _np(o["info"][k]))


@pytest.mark.gpu
def test_zero_steps_and_cold_calls_are_the_ordinary_call():
    tpl, cones, data, warm, _ = _shape("small", 1e-3)
    base_w = _call(tpl, cones, data, warm, {"eps": 1e-6})
    zero_w = _call(tpl, cones, data, warm, {"eps": 1e-6, "newton_first": 0})
    base_c = _call(tpl, cones, data, None, {"eps": 1e-6})
    cold = _call(tpl, cones, data, None, {"eps": 1e-6, "newton_first": 3})
    for a, b in ((base_w, zero_w), (base_c, cold)):
        for k in ("x", "y", "s"):
            np.testing.assert_array_equal(_np(a[k]), _np(b[k]))
        np.testing.assert_array_equal(_np(a["info"]["iters"]), _np(b["info"]["iters"]))
    assert "newton_first" not in zero_w["info"] and "newton_first" not in base_w["info"]
    assert cold["info"]["newton_first"]["path"] == "none" and cold["info"]["newton_first"]["n_accepted"] == 0
    assert (_np(base_w["info"]["iters"]) > 0).all()


@pytest.mark.gpu
def test_a_recording_engine_keeps_the_state_of_full_batch_solves():
    """dispatch history on (the plugin's default): after a cold full-batch solve, a newton_first call with fallbacks leaves the launch plan and what the next
    full-batch solve does exactly as the same call without the feature leaves them"""
    tpl, cones, data, warm, _ = _shape("small", 1e-3, planted=True)
    out = []
    for args in ({"eps": 1e-8, "newton_first": 3}, {"eps": 1e-8}):
        first = _call(tpl, cones, data, None, {"eps": 1e-8})
        assert first["eng"].dispatch_history
        plan0 = first["eng"].plan()
        r = _call(tpl, cones, data, warm, args, ctx=first["ctx"])
        if "newton_first" in args:
            assert 0 < r["info"]["newton_first"]["n_fallback"] < SMALL[2]
        again = _call(tpl, cones, data, None, {"eps": 1e-8}, ctx=first["ctx"])
        out.append((plan0, r["eng"].plan(), r["eng"].last_path, _np(again["x"]), _np(again["info"]["iters"])))
    with_nf, without = out
    assert with_nf[0] == without[0] and with_nf[1] == without[1] and with_nf[2] == without[2] == "per_instance"
    np.testing.assert_array_equal(with_nf[3], without[3]); np.testing.assert_array_equal(with_nf[4], without[4])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["psd", "shared_a"])
def test_templates_without_the_elimination_run_the_ordinary_solve_and_say_so_once(kind, monkeypatch):
    m = _plugin()
    if kind == "psd":
        n, cones, B = 4, {"z": 1, "l": 0, "q": [], "s": [3]}, 5
        data = P.generate(n, cones, B, seed=0)
    else:
        n, cones, B = SMALL[0], SMALL[1], 8
        data = P.generate(n, cones, B, seed=1, batched=("b", "c"))
        monkeypatch.setenv("CE_CONST_A", "1")
    tpl = P.dense_template(n, cones)
    w = oracle.solve_batch(*data, cones, eps=1e-4)
    warm = (w["x"], w["y"], w["s"])
    base = _call(tpl, cones, data, warm, {"eps": 1e-6})
    m._WARNED.discard("newton_first_none")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        r1 = _call(tpl, cones, data, warm, {"eps": 1e-6, "newton_first": 2})
        r2 = _call(tpl, cones, data, warm, {"eps": 1e-6, "newton_first": 2})
    said = [str(x.message) for x in rec if "newton_first" in str(x.message)]
    assert len(said) == 1, said
    assert base["eng"].last_path == ("const_a" if kind == "shared_a" else "per_instance") == r1["eng"].last_path
    for r in (r1, r2):
        nf = r["info"]["newton_first"]
        assert nf["path"] == "none" and nf["n_accepted"] == 0 and nf["n_fallback"] == B and nf["accepted"] is None
        for k in ("x", "y", "s"):
            np.testing.assert_array_equal(_np(r[k]), _np(base[k]))
        np.testing.assert_array_equal(_np(r["info"]["iters"]), _np(base["info"]["iters"]))

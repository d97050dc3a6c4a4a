"""The solver_args keys of PSD templates on a template with PSD blocks AND exponential / power triples (interfaces/mi355_if.py): on a mixed template that the plan
serves, psd_elimination="search_free" gives jvp_mode="direct" (ce_jvp_psd_tri), refine_steps and newton_first (ce_refine_psd_tri); psd_adjoint="search_free" the
reverse Jacobian by ce_vjp_psd_tri_many; psd_tangents="many" the forward Jacobian by ce_jvp_psd_tri_many.  tri_adjoint / tri_tangents stay inert beside a PSD
block.  With the keys absent every output, warning and info entry is what it is with the keys at their defaults.
Templates: psd_tri_ns_kit's mix_all through the plugin's autograd function (test_gpu_psd_ns_layer.py::_call), and a CvxpyLayer(template=...) whose parameters are
the solver-form A, b, c of mix_small, all batched, built as tests/ref_cases.py builds its cases (outputs: x and the dual)."""
import warnings

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import psd_tri_ns_kit as K
from cvxpylayers_amd import problems as P
from newton_first_kit import perturb
from oracle import oracle

pytestmark = pytest.mark.gpu
TIGHT = {"lsqr_atol": 1e-12, "lsqr_btol": 1e-12, "lsqr_iter_lim": 20000}          # kit.TIGHT_LSQR as solver_args
ELIM, ADJ, TAN = {"psd_elimination": "search_free"}, {"psd_adjoint": "search_free"}, {"psd_tangents": "many"}
DEFAULTS = {"psd_elimination": "off", "psd_adjoint": "pivoting", "psd_tangents": "loop"}
_CACHE: dict = {}


def _plugin():
    from cvxpylayers_amd.interfaces import mi355_if
    return mi355_if


def _np(t):
    return t.detach().cpu().numpy()


def _call(args, warm=None, data=None):
    """one call of the plugin's autograd function on mix_all (a fresh context and engine per call: no warm-start memory between calls)"""
    m = _plugin()
    n, cones, A, b, c, _ = K.problem("mix_all")
    tpl = P.dense_template(n, cones)
    dev = torch.device("cuda", 0)
    ctx = m.MI355_ctx(None, tpl.problem_data_index, cones)
    A_eval, q_eval = tpl.values_from_dense(*(data or (A, b, c)))
    A_t, q_t = torch.from_numpy(A_eval).to(dev), torch.from_numpy(q_eval).to(dev)
    w = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in warm) if warm is not None else None
    primal, dual, info, _ = m._CvxpyLayer.apply(None, q_t, A_t, ctx, dict(args), False, w)
    torch.cuda.synchronize()
    return dict(x=primal, y=dual, info=info, eng=ctx.engine(dev))


def _layer():
    """the CvxpyLayer on mix_small with parameters (A, b, c), its engine and the Jacobians every test compares: computed once, shared, not changed"""
    if _CACHE:
        return _CACHE
    from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    n, cones, A, b, c, _ = K.problem("mix_small")
    m = K.m_of(cones)
    tpl = template_from_affine_builder(lambda A, b, c: (A, b, c), [(m, n), (m,), (n,)], cones,
                                       [VariableRecovery(slice(0, n), None, (n,)), VariableRecovery(None, slice(0, m), (m,), source="dual")])
    layer = CvxpyLayer(template=tpl, solver_args={"eps": 1e-9, "max_iters": 200000, **TIGHT})
    params = tuple(torch.from_numpy(p).cuda() for p in (A, b, c))
    layer(*params)
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert eng.psd_tri_ns_variant == K.PLAN["mix_small"][0] and eng.psd_ns_variant == -1
    runs = {}
    for name, kw in (("default", {}), ("adj", dict(solver_args=ADJ)), ("fwd_default", dict(direction="forward")), ("tan", dict(direction="forward", solver_args=TAN))):
        eng.last_vjp_many_path = eng.last_vjp_kernel = eng.last_jvp_many_path = eng.last_jvp_kernel = "untouched"
        outs, jac = layer.jacobian(*params, **kw)
        runs[name] = dict(outs=outs, jac=jac, vjp=(eng.last_vjp_many_path, eng.last_vjp_kernel), jvp=(eng.last_jvp_many_path, eng.last_jvp_kernel),
                          adjoint=dict(layer.info["adjoint"]), fwd=dict(layer.info.get("jvp") or {}))
    _CACHE.update(layer=layer, eng=eng, params=params, runs=runs, B=int(A.shape[0]))
    return _CACHE


def _agree(jac, want, sel, what):
    assert len(jac) == len(want)
    for i in range(len(jac)):
        for j in range(len(jac[i])):
            got, w = jac[i][j][sel], want[i][j][sel]
            assert got.shape == w.shape and float(w.abs().max()) > 1e-3
            e = float((got - w).abs().max() / (1 + w.abs().max()))
            print(f"{what} jac[{i}][{j}] against the default route: {e:.2e}")
            assert e < 1e-6, (what, i, j, e)


def test_forward_ad_names_ce_jvp_psd_tri_under_the_two_keys_and_equals_the_lsqr_route():
    """fails on a tree without the mode: the call under the two keys runs ce_jvp_lsqr there"""
    c = _layer()
    layer, (A0, b0, c0) = c["layer"], c["params"]
    gen = torch.Generator(device="cpu").manual_seed(5)
    tans = tuple(torch.randn(p.shape, generator=gen, dtype=torch.float64).cuda() for p in (A0, b0, c0))
    got = {}
    with fwAD.dual_level():
        for name, args in (("mixed", {"jvp_mode": "direct", **ELIM}), ("lsqr", {}), ("direct_without_the_key", {"jvp_mode": "direct"}), ("tri_keys", {"jvp_mode": "direct", "tri_tangents": "many"})):
            outs = layer(*(fwAD.make_dual(p.clone(), t) for p, t in zip((A0, b0, c0), tans)), solver_args=args)
            info = layer.info["jvp"]
            got[name] = ([fwAD.unpack_dual(o).tangent.detach().clone() for o in outs], [fwAD.unpack_dual(o).primal.detach().clone() for o in outs],
                         info["kernel"], info["path"], _np(info["status"]), _np(info["iters"]))
    assert got["mixed"][2:4] == ("ce_jvp_psd_tri", "direct"), got["mixed"][2:4]
    for name in ("lsqr", "direct_without_the_key", "tri_keys"):          # today's routes
        assert got[name][2:4] == ("ce_jvp_lsqr", "lsqr"), (name, got[name][2:4])
    st, its = got["mixed"][4], got["mixed"][5]
    print("ce_jvp_psd_tri status", st, "iters", its, "lsqr status", got["lsqr"][4])
    assert (got["lsqr"][4] == 0).all()
    reg = st == 0
    assert reg.mean() >= 0.8 and (its[reg] == 0).all() and (its[~reg] > 0).all()
    for k, name in enumerate(("x", "dual")):
        a, l = _np(got["mixed"][0][k]).reshape(st.size, -1), _np(got["lsqr"][0][k]).reshape(st.size, -1)
        e = (np.abs(a - l).max(axis=1) / (1 + np.abs(l).max(axis=1)))[reg]
        print(f"tangent of {name}: max {e.max():.3e} median {np.median(e):.3e}; max |tangent| {np.abs(l).max():.3e}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, e.max(), np.median(e))
        assert np.abs(l).max() > 1e-3
    for k in range(2):          # the key changes nothing of the forward solve, and without it the tangents are today's, bit for bit
        assert torch.equal(got["mixed"][1][k], got["lsqr"][1][k])
        assert torch.equal(got["direct_without_the_key"][0][k], got["lsqr"][0][k]) and torch.equal(got["tri_keys"][0][k], got["lsqr"][0][k])


def test_refine_steps_are_served_with_no_notice_and_land_closer_to_the_oracle():
    hi = K.problem("mix_all")[5]
    _plugin()._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        r1 = _call({"eps": 1e-4, "refine_steps": 2, **ELIM})
    assert not [str(x.message) for x in rec if "refine_steps" in str(x.message) or "psd_elimination" in str(x.message)], [str(x.message) for x in rec]
    r0 = _call({"eps": 1e-4})
    assert r1["info"]["refine"]["path"] == "ns" and "refine" not in r0["info"]
    d1, d0 = (np.abs(_np(r["x"]) - hi["x"]).max(axis=1) for r in (r1, r0))
    st = _np(r1["info"]["refine"]["status"])
    print(f"refine status {np.bincount(st)}; max |x - oracle|: refined median {np.median(d1):.3e} max {d1.max():.3e}, unrefined median {np.median(d0):.3e} max {d0.max():.3e}")
    assert (d1 < d0).all(), (d1, d0)


def test_newton_first_accepts_instances_and_equals_the_cold_solve():
    """the warm start is the oracle's eps = 1e-6 point of the unperturbed data; the call's data is that data with every entry moved by 0.1 % (newton_first_kit.perturb);
    against the cold solve of the same data at the same eps under the project's eps = 1e-8 parity gate, 1e-6 (1 + |.|_inf)"""
    n, cones, A0, b0, c0, _ = K.problem("mix_all")
    data = perturb(A0, b0, c0, 1e-3, K.SHAPES["mix_all"][3])
    w = oracle.solve_batch(A0, b0, c0, cones, eps=1e-6)
    assert (w["status"] == 1).all()
    r = _call({"eps": 1e-8, "newton_first": 2, **ELIM}, warm=(w["x"], w["y"], w["s"]), data=data)
    cold = _call({"eps": 1e-8}, data=data)
    nf = r["info"]["newton_first"]
    print(f"accepted {nf['n_accepted']}, fallback {nf['n_fallback']}")
    assert nf["path"] == "ns" and nf["steps"] == 2 and nf["refine"]["path"] == "ns" and nf["n_accepted"] > 0
    assert (_np(r["info"]["status"]) == 1).all() and (_np(cold["info"]["status"]) == 1).all()
    assert (_np(r["info"]["iters"])[_np(nf["accepted"])] == 0).all()
    for k in ("x", "y"):
        got, want = _np(r[k]), _np(cold[k])
        err = np.abs(got - want).max(axis=1); gate = 1e-6 * (1 + np.abs(want).max(axis=1))
        print(f"    max |{k} - cold| / gate = {(err / gate).max():.3e}")
        assert (err <= gate).all(), (k, err.max())
    off = _call({"eps": 1e-8, "newton_first": 2}, warm=(w["x"], w["y"], w["s"]), data=data)          # without the key the same call is today's: not served
    assert off["info"]["newton_first"]["path"] == "none"


def test_the_reverse_jacobian_names_ce_vjp_psd_tri_many_and_agrees_with_the_default():
    c = _layer()
    d, a = c["runs"]["default"], c["runs"]["adj"]
    assert d["vjp"] == ("loop", None) and d["adjoint"]["path"] != "ce_vjp_psd_tri_many"          # today's route without the key
    assert a["vjp"] == ("many", "ce_vjp_psd_tri_many") and a["adjoint"]["path"] == "ce_vjp_psd_tri_many"
    st_a, st_d = a["adjoint"]["status"].cpu().numpy(), d["adjoint"]["status"].cpu().numpy()
    assert st_a.shape == st_d.shape and st_a.shape[1] == c["B"]
    both = ((st_a == 0) & (st_d == 0)).all(axis=0)
    print("status under the key", np.bincount(st_a.ravel()).tolist(), "default", np.bincount(st_d.ravel()).tolist(), "instances unflagged by both", int(both.sum()), "of", c["B"])
    assert both.mean() >= 0.8, (st_a, st_d)
    assert all(torch.equal(u, v) for u, v in zip(a["outs"], d["outs"]))
    _agree(a["jac"], d["jac"], torch.from_numpy(both).cuda(), "psd_adjoint")


def test_the_forward_jacobian_names_ce_jvp_psd_tri_many_and_agrees_with_the_default():
    c = _layer()
    f, t = c["runs"]["fwd_default"], c["runs"]["tan"]
    assert f["jvp"] == ("loop", "ce_jvp_lsqr") and f["fwd"]["kernel"] == "ce_jvp_lsqr" and f["fwd"]["path"] == "lsqr"          # today's route without the key
    assert t["jvp"] == ("many", "ce_jvp_psd_tri_many") and t["fwd"]["kernel"] == "ce_jvp_psd_tri_many" and t["fwd"]["path"] == "direct"
    st_t, st_f = t["fwd"]["status"].cpu().numpy(), f["fwd"]["status"].cpu().numpy()
    both = (st_t == 0).all(axis=0) & (st_f == 0).all(axis=0)
    print("status under the key", np.bincount(st_t.ravel()).tolist(), "instances unflagged by both", int(both.sum()), "of", c["B"])
    assert both.mean() >= 0.8, (st_t, st_f)
    assert all(torch.equal(u, v) for u, v in zip(t["outs"], f["outs"]))
    _agree(t["jac"], f["jac"], torch.from_numpy(both).cuda(), "psd_tangents")
    _agree(t["jac"], c["runs"]["default"]["jac"], torch.from_numpy(both).cuda(), "psd_tangents against the default reverse Jacobian")


def test_the_triples_keys_stay_inert_beside_a_psd_block():
    c = _layer()
    layer, eng = c["layer"], c["eng"]
    want = c["runs"]["default"]["jac"]
    _, jac = layer.jacobian(*c["params"], solver_args={"tri_adjoint": "search_free", "tri_tangents": "many"})
    assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None
    assert all(torch.equal(jac[i][j], want[i][j]) for i in range(len(want)) for j in range(len(want[i])))
    _, jac = layer.jacobian(*c["params"], direction="forward", solver_args={"tri_adjoint": "search_free", "tri_tangents": "many"})
    assert (eng.last_jvp_many_path, eng.last_jvp_kernel) == ("loop", "ce_jvp_lsqr")
    want = c["runs"]["fwd_default"]["jac"]
    assert all(torch.equal(jac[i][j], want[i][j]) for i in range(len(want)) for j in range(len(want[i])))


def _same_info(a, b, path=""):
    assert type(a) is type(b) or (a is None) == (b is None), (path, type(a), type(b))
    if isinstance(a, dict):
        assert set(a) == set(b), (path, set(a) ^ set(b))
        for k in a:
            _same_info(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, torch.Tensor):
        assert torch.equal(a, b) or (a.is_floating_point() and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))), path
    elif isinstance(a, (int, float, str, bool, type(None), tuple)):
        assert a == b or (isinstance(a, float) and a != a and b != b), (path, a, b)


def test_with_no_key_outputs_warnings_and_info_equal_a_run_with_the_keys_at_their_defaults():
    outs = []
    for args in ({"eps": 1e-6, "refine_steps": 1}, {"eps": 1e-6, "refine_steps": 1, **DEFAULTS}):
        _plugin()._WARNED.clear()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            r = _call(args)
        outs.append((r, sorted(str(x.message) for x in rec)))
    (a, wa), (b, wb) = outs
    assert wa == wb and [w for w in wa if "refine_steps" in w], (wa, wb)          # today's notice, the same in both: the steps are not served without the key
    assert a["info"]["refine"]["path"] == "none"
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["y"], b["y"])
    _same_info(a["info"], b["info"])
    c = _layer()
    layer = c["layer"]
    _, jac = layer.jacobian(*c["params"], solver_args=DEFAULTS)
    info_d = {k: (dict(v) if isinstance(v, dict) else v) for k, v in layer.info.items()}
    _, jac0 = layer.jacobian(*c["params"])
    assert all(torch.equal(jac[i][j], jac0[i][j]) for i in range(len(jac)) for j in range(len(jac[i])))
    _same_info(info_d, {k: (dict(v) if isinstance(v, dict) else v) for k, v in layer.info.items()})

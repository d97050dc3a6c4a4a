"""solver_args psd_elimination="search_free" through the layer (interfaces/mi355_if.py): a per-instance-A template with PSD blocks gets forward-mode AD by
ce_jvp_psd under jvp_mode="direct", refine_steps and newton_first by ce_refine_psd; with the key absent (or "off") every output and info entry is what it was.
Templates: ref_cases.case_sdp_symmetric_primal_and_psd_dual() (min tr(C X), tr X = 1, X PSD of order 4) through CvxpyLayer, and psd_ns_kit's lqr_like
(PSD(6) + PSD(4) beside zero and nonnegative rows) through the plugin's autograd function, as test_gpu_newton_first.py calls it."""
import warnings

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import psd_ns_kit as K
import ref_cases
from cvxpylayers_amd import problems as P
from newton_first_kit import perturb
from oracle import oracle

pytestmark = pytest.mark.gpu
TIGHT = {"lsqr_atol": 1e-12, "lsqr_btol": 1e-12, "lsqr_iter_lim": 20000}          # kit.TIGHT_LSQR as solver_args
_CACHE: dict = {}


def _plugin():
    from cvxpylayers_amd.interfaces import mi355_if
    return mi355_if


def _np(t):
    return t.detach().cpu().numpy()


def _call(args, warm=None, data=None, dual_tangents=None):
    """one call of the plugin's autograd function on lqr_like (a fresh context and engine per call: no warm-start memory between calls)"""
    m = _plugin()
    n, cones, A, b, c, _ = K.problem("lqr_like")
    tpl = P.dense_template(n, cones)
    dev = torch.device("cuda", 0)
    ctx = m.MI355_ctx(None, tpl.problem_data_index, cones)
    A_eval, q_eval = tpl.values_from_dense(*(data or (A, b, c)))
    A_t, q_t = torch.from_numpy(A_eval).to(dev), torch.from_numpy(q_eval).to(dev)
    w = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in warm) if warm is not None else None
    primal, dual, info, _ = m._CvxpyLayer.apply(None, q_t, A_t, ctx, dict(args), False, w)
    torch.cuda.synchronize()
    return dict(x=primal, y=dual, info=info, eng=ctx.engine(dev))


def test_forward_ad_names_ce_jvp_psd_and_equals_the_lsqr_route():
    """the SDP case at eps 1e-9 under the tight LSQR rule: the tangents of X and of the PSD constraint's dual by ce_jvp_psd against the same call under the default
    jvp_mode (ce_jvp_lsqr), to the bounds of test_gpu_jvp_direct._check_regular_against_lsqr over the directly solved instances (all of them: B = 3)"""
    from cvxpylayers_amd.torch import CvxpyLayer
    cs = ref_cases.case_sdp_symmetric_primal_and_psd_dual()
    base = {"eps": 1e-9, "max_iters": 200000, **TIGHT}
    layer = CvxpyLayer(template=cs["template"], solver_args=base)
    C0 = torch.from_numpy(cs["params"][0]).cuda()
    gen = torch.Generator(device="cpu").manual_seed(5)
    tC = torch.randn(C0.shape, generator=gen, dtype=torch.float64); tC = (0.5 * (tC + tC.transpose(1, 2))).cuda()
    got = {}
    with fwAD.dual_level():
        for name, args in (("psd", {"jvp_mode": "direct", "psd_elimination": "search_free"}), ("lsqr", {}), ("direct_without_the_key", {"jvp_mode": "direct"})):
            outs = layer(fwAD.make_dual(C0.clone(), tC), solver_args=args)
            info = layer.info["jvp"]
            got[name] = ([fwAD.unpack_dual(o).tangent.detach().clone() for o in outs], [fwAD.unpack_dual(o).primal.detach().clone() for o in outs],
                         info["kernel"], info["path"], _np(info["status"]), _np(info["iters"]))
    assert got["psd"][2:4] == ("ce_jvp_psd", "direct"), got["psd"][2:4]
    assert got["lsqr"][2:4] == ("ce_jvp_lsqr", "lsqr") and got["direct_without_the_key"][2:4] == ("ce_jvp_lsqr", "lsqr")          # today's routes
    st, its = got["psd"][4], got["psd"][5]
    print("ce_jvp_psd status", st, "iters", its, "lsqr status", got["lsqr"][4], "iters", got["lsqr"][5])
    assert (got["lsqr"][4] == 0).all()
    reg = st == 0
    assert reg.mean() >= 0.8 and (its[reg] == 0).all() and (its[~reg] > 0).all()
    for k, name in enumerate(("X", "dual")):
        a, l = _np(got["psd"][0][k]).reshape(st.size, -1), _np(got["lsqr"][0][k]).reshape(st.size, -1)
        e = (np.abs(a - l).max(axis=1) / (1 + np.abs(l).max(axis=1)))[reg]
        print(f"tangent of {name}: max {e.max():.3e} median {np.median(e):.3e}; max |tangent| {np.abs(l).max():.3e}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, e.max(), np.median(e))
        assert np.abs(l).max() > 1e-3
    for k in range(2):          # the key changes nothing of the forward solve, and without it the tangents are today's, bit for bit
        assert torch.equal(got["psd"][1][k], got["lsqr"][1][k])
        assert torch.equal(got["direct_without_the_key"][0][k], got["lsqr"][0][k])


def test_refine_steps_are_served_and_land_closer_to_the_oracle():
    hi = K.problem("lqr_like")[5]
    _plugin()._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        r1 = _call({"eps": 1e-4, "refine_steps": 2, "psd_elimination": "search_free"})
    assert not [str(x.message) for x in rec if "refine_steps" in str(x.message) or "psd_elimination" in str(x.message)]
    r0 = _call({"eps": 1e-4})
    assert r1["info"]["refine"]["path"] == "ns" and "refine" not in r0["info"]
    d1, d0 = (np.abs(_np(r["x"]) - hi["x"]).max(axis=1) for r in (r1, r0))
    st = _np(r1["info"]["refine"]["status"])
    print(f"refine status {np.bincount(st)}; max |x - oracle|: refined median {np.median(d1):.3e} max {d1.max():.3e}, unrefined median {np.median(d0):.3e} max {d0.max():.3e}")
    assert (d1 < d0).all(), (d1, d0)


def test_newton_first_accepts_instances_and_equals_the_cold_solve():
    """the warm start is the oracle's eps = 1e-6 point of the unperturbed data; the call's data is that data with every entry moved by 0.1 % (newton_first_kit.perturb);
    against the cold solve of the same data at the same eps under the project's eps = 1e-8 parity gate, 1e-6 (1 + |.|_inf)"""
    n, cones, A0, b0, c0, _ = K.problem("lqr_like")
    data = perturb(A0, b0, c0, 1e-3, K.SHAPES["lqr_like"][3])
    w = oracle.solve_batch(A0, b0, c0, cones, eps=1e-6)
    assert (w["status"] == 1).all()
    r = _call({"eps": 1e-8, "newton_first": 2, "psd_elimination": "search_free"}, warm=(w["x"], w["y"], w["s"]), data=data)
    cold = _call({"eps": 1e-8}, data=data)
    nf = r["info"]["newton_first"]
    print(f"accepted {nf['n_accepted']}, fallback {nf['n_fallback']}, iters of the fallback instances {_np(r['info']['iters'])[~_np(nf['accepted'])]}")
    assert nf["path"] == "ns" and nf["steps"] == 2 and nf["refine"]["path"] == "ns" and nf["n_accepted"] > 0
    assert (_np(r["info"]["status"]) == 1).all() and (_np(cold["info"]["status"]) == 1).all()
    assert (_np(r["info"]["iters"])[_np(nf["accepted"])] == 0).all()
    for k in ("x", "y"):
        got, want = _np(r[k]), _np(cold[k])
        err = np.abs(got - want).max(axis=1); gate = 1e-6 * (1 + np.abs(want).max(axis=1))
        print(f"    max |{k} - cold| / gate = {(err / gate).max():.3e}")
        assert (err <= gate).all(), (k, err.max())
    # without the key the same call is today's: not served
    off = _call({"eps": 1e-8, "newton_first": 2}, warm=(w["x"], w["y"], w["s"]), data=data)
    assert off["info"]["newton_first"]["path"] == "none"


def test_with_the_key_absent_or_off_everything_is_as_it_was():
    _plugin()._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        a = _call({"eps": 1e-6, "refine_steps": 1})
        b = _call({"eps": 1e-6, "refine_steps": 1, "psd_elimination": "off"})
    assert [str(x.message) for x in rec if "refine_steps" in str(x.message)]          # today's notice: the steps are not served
    assert a["info"]["refine"]["path"] == "none" and b["info"]["refine"]["path"] == "none"
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["y"], b["y"])
    assert set(a["info"]) == set(b["info"]) and set(a["info"]["refine"]) == set(b["info"]["refine"])
    c = _call({"eps": 1e-6})
    d = _call({"eps": 1e-6, "psd_elimination": "search_free"})          # nothing asks for the elimination: the key alone changes no output
    assert torch.equal(c["x"], d["x"]) and torch.equal(c["y"], d["y"]) and torch.equal(c["x"], a["x"]) and set(c["info"]) == set(d["info"])
    # a plain template: the key is inert and silent
    m = _plugin()
    n, cones = 12, {"z": 2, "l": 8, "q": [4, 5]}
    A, bb, cc = P.generate(n, cones, 8, seed=1)
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, bb, cc)
    outs = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for args in ({"eps": 1e-6, "refine_steps": 1}, {"eps": 1e-6, "refine_steps": 1, "psd_elimination": "search_free"}):
            ctx = m.MI355_ctx(None, tpl.problem_data_index, cones)
            outs.append(m._CvxpyLayer.apply(None, torch.from_numpy(q_eval).cuda(), torch.from_numpy(A_eval).cuda(), ctx, args, False, None))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[1][2]["refine"]["path"] == "ns"

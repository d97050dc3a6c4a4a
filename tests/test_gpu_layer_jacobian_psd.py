"""CvxpyLayer.jacobian on a layer with PSD blocks under solver_args psd_adjoint="search_free" (reverse: one ce_vjp_psd_many call per chunk instead of the loop of
pivoting ce_vjp calls) and psd_tangents="many" (forward: one ce_jvp_psd_many call per chunk instead of the loop of single-tangent calls).

The layer is test_gpu_psd_ns_layer.py's SDP: ref_cases.case_sdp_symmetric_primal_and_psd_dual() (min tr(C X), tr X = 1, X PSD of order 4; B = 3; outputs X and the
PSD constraint's dual) at eps 1e-9 under the tight LSQR rule.  Both Jacobians under the keys agree with the default reverse Jacobian within 1e-6 relative
(test_gpu_layer_jacobian.py's bound) on the instances no route flags; info names the entry points; chunking by a small max_bytes gives the one-chunk result;
.backward() and one-tangent forward-mode AD ignore the keys; without the keys the routes and outputs are today's."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import ref_cases

pytestmark = pytest.mark.gpu
TIGHT = {"lsqr_atol": 1e-12, "lsqr_btol": 1e-12, "lsqr_iter_lim": 20000}          # kit.TIGHT_LSQR as solver_args
ADJ, TAN = {"psd_adjoint": "search_free"}, {"psd_tangents": "many"}
_CACHE: dict = {}


def _setup():
    """the layer, its parameter and the Jacobians every test compares: computed once, shared, not changed"""
    if _CACHE:
        return _CACHE
    from cvxpylayers_amd.torch import CvxpyLayer
    cs = ref_cases.case_sdp_symmetric_primal_and_psd_dual()
    layer = CvxpyLayer(template=cs["template"], solver_args={"eps": 1e-9, "max_iters": 200000, **TIGHT})
    params = tuple(torch.from_numpy(p).cuda() for p in cs["params"])
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert eng.psd_ns_variant >= 0
    runs = {}
    for name, kw in (("default", {}), ("adj", dict(solver_args=ADJ)), ("fwd_default", dict(direction="forward")), ("tan", dict(direction="forward", solver_args=TAN))):
        eng.last_vjp_many_path = eng.last_vjp_kernel = eng.last_jvp_many_path = eng.last_jvp_kernel = "untouched"
        outs, jac = layer.jacobian(*params, **kw)
        runs[name] = dict(outs=outs, jac=jac, vjp=(eng.last_vjp_many_path, eng.last_vjp_kernel), jvp=(eng.last_jvp_many_path, eng.last_jvp_kernel),
                          adjoint=dict(layer.info["adjoint"]), fwd=dict(layer.info.get("jvp") or {}))
    _CACHE.update(layer=layer, eng=eng, params=params, runs=runs, B=int(params[0].shape[0]))
    return _CACHE


def _agree(jac, want, sel, what):
    assert len(jac) == len(want)
    for i in range(len(jac)):
        for j in range(len(jac[i])):
            got, w = jac[i][j][sel], want[i][j][sel]
            assert got.shape == w.shape and float(w.abs().max()) > 1e-3
            e = float((got - w).abs().max() / (1 + w.abs().max()))
            print(f"{what} jac[{i}][{j}] against the default reverse Jacobian: {e:.2e}")
            assert e < 1e-6, (what, i, j, e)


def test_the_search_free_reverse_jacobian_names_ce_vjp_psd_many_and_agrees_with_the_default():
    """fails on a tree without the mode: psd_adjoint is not a known solver argument there, and the call under it runs the loop"""
    c = _setup()
    d, a = c["runs"]["default"], c["runs"]["adj"]
    assert d["vjp"] == ("loop", None) and d["adjoint"]["path"] != "ce_vjp_psd_many"          # today's route without the key
    assert a["vjp"] == ("many", "ce_vjp_psd_many") and a["adjoint"]["path"] == "ce_vjp_psd_many"
    st_a, st_d = a["adjoint"]["status"].cpu().numpy(), d["adjoint"]["status"].cpu().numpy()
    assert st_a.shape == st_d.shape and st_a.shape[1] == c["B"]
    both = ((st_a == 0) & (st_d == 0)).all(axis=0)
    print("status under the key", np.bincount(st_a.ravel()).tolist(), "default", np.bincount(st_d.ravel()).tolist(), "instances unflagged by both", int(both.sum()), "of", c["B"])
    assert both.mean() >= 0.5, (st_a, st_d)
    assert all(torch.equal(u, v) for u, v in zip(a["outs"], d["outs"]))
    _agree(a["jac"], d["jac"], torch.from_numpy(both).cuda(), "psd_adjoint")


def test_the_many_tangent_forward_jacobian_names_ce_jvp_psd_many_and_agrees_with_the_reverse():
    c = _setup()
    d, f, t = c["runs"]["default"], c["runs"]["fwd_default"], c["runs"]["tan"]
    assert f["jvp"] == ("loop", "ce_jvp_lsqr") and f["fwd"]["kernel"] == "ce_jvp_lsqr" and f["fwd"]["path"] == "lsqr"          # today's route without the key
    assert t["jvp"] == ("many", "ce_jvp_psd_many") and t["fwd"]["kernel"] == "ce_jvp_psd_many" and t["fwd"]["path"] == "direct"
    st_t, st_d = t["fwd"]["status"].cpu().numpy(), d["adjoint"]["status"].cpu().numpy()
    both = (st_t == 0).all(axis=0) & (st_d == 0).all(axis=0)
    print("status under the key", np.bincount(st_t.ravel()).tolist(), "instances unflagged by both", int(both.sum()), "of", c["B"])
    assert both.mean() >= 0.5, (st_t, st_d)
    assert all(torch.equal(u, v) for u, v in zip(t["outs"], d["outs"]))
    _agree(t["jac"], d["jac"], torch.from_numpy(both).cuda(), "psd_tangents")


def test_several_chunks_give_the_one_chunk_result():
    c = _setup()
    layer, eng, B = c["layer"], c["eng"], c["B"]
    calls = []
    orig = eng.vjp_many
    eng.vjp_many = lambda *a, **kw: (calls.append(int(a[4].shape[0])), orig(*a, **kw))[1]
    try:
        _, jac_c = layer.jacobian(*c["params"], solver_args=ADJ, max_bytes=5 * B * eng.nnz_aug * 8)
    finally:
        del eng.vjp_many
    assert len(calls) > 2 and max(calls) == 5 and eng.last_vjp_kernel == "ce_vjp_psd_many", calls
    want = c["runs"]["adj"]["jac"]
    assert all(torch.equal(jac_c[i][j], want[i][j]) for i in range(len(want)) for j in range(len(want[i])))
    calls = []
    orig = eng.jvp_many
    eng.jvp_many = lambda *a, **kw: (calls.append(int(a[5].shape[0])), orig(*a, **kw))[1]
    try:
        _, jac_c = layer.jacobian(*c["params"], direction="forward", solver_args=TAN, max_bytes=5 * B * (eng.n + 2 * eng.m) * 8)
    finally:
        del eng.jvp_many
    assert len(calls) > 2 and max(calls) == 5 and eng.last_jvp_kernel == "ce_jvp_psd_many", calls
    want = c["runs"]["tan"]["jac"]
    assert all(torch.equal(jac_c[i][j], want[i][j]) for i in range(len(want)) for j in range(len(want[i])))


def test_the_default_values_keep_their_routes_and_a_third_value_is_refused():
    c = _setup()
    layer, eng = c["layer"], c["eng"]
    _, jac_p = layer.jacobian(*c["params"], solver_args={"psd_adjoint": "pivoting", "psd_tangents": "loop"})
    assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None
    want = c["runs"]["default"]["jac"]
    assert all(torch.equal(jac_p[i][j], want[i][j]) for i in range(len(want)) for j in range(len(want[i])))
    # the keys are independent of psd_elimination: under it the many routes keep their loops, bit for bit
    _, jac_e = layer.jacobian(*c["params"], solver_args={"psd_elimination": "search_free"})
    assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None
    assert all(torch.equal(jac_e[i][j], want[i][j]) for i in range(len(want)) for j in range(len(want[i])))
    # each key acts on its own direction alone
    _, jac_x = layer.jacobian(*c["params"], solver_args=TAN)
    assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None
    assert all(torch.equal(jac_x[i][j], want[i][j]) for i in range(len(want)) for j in range(len(want[i])))
    for key in ("psd_adjoint", "psd_tangents"):
        with pytest.raises(ValueError, match=key):
            layer.jacobian(*c["params"], solver_args={key: "search-free"})


def test_backward_and_one_tangent_forward_ad_ignore_the_keys():
    c = _setup()
    layer, eng = c["layer"], c["eng"]
    both = {**ADJ, **TAN}
    grads = []
    for args in ({}, both):
        ps = [p.clone().requires_grad_(True) for p in c["params"]]
        outs = layer(*ps, solver_args=args)
        eng.last_vjp_kernel = "untouched"
        sum((o * torch.arange(1, o.numel() + 1, dtype=o.dtype, device=o.device).reshape(o.shape)).sum() for o in outs).backward()
        assert eng.last_vjp_kernel == "untouched" and layer.info["adjoint"]["path"] != "ce_vjp_psd_many"
        grads.append([p.grad for p in ps])
    for g0, g1 in zip(*grads):
        assert g0 is not None and torch.equal(g0, g1)
    C0 = c["params"][0]
    gen = torch.Generator(device="cpu").manual_seed(5)
    tC = torch.randn(C0.shape, generator=gen, dtype=torch.float64); tC = (0.5 * (tC + tC.transpose(1, 2))).cuda()
    tans = []
    with fwAD.dual_level():
        for args in ({"jvp_mode": "direct"}, {"jvp_mode": "direct", **both}):
            outs = layer(fwAD.make_dual(C0.clone(), tC), solver_args=args)
            assert layer.info["jvp"]["kernel"] == "ce_jvp_lsqr"          # (without psd_elimination a PSD template's one tangent is the LSQR call, as ever)
            tans.append([fwAD.unpack_dual(o).tangent.detach().clone() for o in outs])
    for t0, t1 in zip(*tans):
        assert torch.equal(t0, t1) and float(t0.abs().max()) > 0

"""The forward-mode derivative by direct elimination: k_backward_ns<..., FWD> behind ce_jvp, ConeEngine.jvp(method="direct"), solver_args jvp_mode="direct".
The same search-free null-space elimination as the default adjoint on the transposed block, with diffcp's LSQR behind it on the device for the instances it
flags rank deficient.  Checked against
  * the LSQR forward derivative (ce_jvp_lsqr) under the tight rule on the same tangents, per variant of the kernel, to the bounds the adjoint's elimination is
    held to (test_gpu_ns_adjoint.py::_check_regular: 1e-5 maximum, 1e-8 median, relative to 1 + max |reference|);
  * the transpose identity against the search-free adjoint the oracle pins;
  * central differences of the GPU solve;
  * duplicated equality rows and LP vertices: flagged (status 4 | 8), re-solved, equal to the LSQR call;
  * null tangents, the plugin's jvp_mode and its fallback where the template has no elimination.
"Regular" below: jvp_status == 0 on the direct path; "flagged": bit 8 set.  All linearisation points are the oracle's solutions (instances the oracle does not
solve are left out, as in test_gpu_ns_adjoint.py)."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import ref_cases
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_jvp import _closed_form, _engine, _tangents

pytestmark = pytest.mark.gpu


def _point(n, cones, B, seed, eps=1e-9, min_solved=0.9, mutate=None):
    """template, engine, batch-major values, q_eval, the oracle's (x, y, s) on the device and the tangents, for the instances the oracle solves"""
    from oracle import oracle
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=seed)
    extra = mutate(A, b) if mutate is not None else None
    ref = oracle.solve_batch(A, b, c, cones, eps=eps, max_iters=200000)
    keep = ref["status"] == 1
    assert keep.mean() >= min_solved, keep.mean()
    A_eval, q_eval = tpl.values_from_dense(A[keep], b[keep], c[keep])
    eng = _engine(tpl)
    A_bm = torch.from_numpy(A_eval).cuda().t().contiguous()
    pt = tuple(torch.from_numpy(ref[k][keep]).cuda() for k in ("x", "y", "s"))
    _, tA_bm, tq = _tangents(tpl, int(keep.sum()), seed=seed + 100)
    return dict(tpl=tpl, eng=eng, A_bm=A_bm, q_t=torch.from_numpy(q_eval).cuda(), pt=pt, tA_bm=tA_bm, tq=tq, keep=keep, extra=extra)


def _both(r, tA_bm="given", tq="given"):
    """(dx, dy, ds, status, iters) as numpy arrays of the direct call and of the LSQR call under the tight rule, on the same tangents"""
    eng = r["eng"]
    tA_bm = r["tA_bm"] if isinstance(tA_bm, str) else tA_bm
    tq = r["tq"] if isinstance(tq, str) else tq
    out = {}
    for method, kernel in (("direct", "ce_jvp"), ("lsqr", "ce_jvp_lsqr")):
        got = eng.jvp(r["A_bm"], *r["pt"], tA_bm, tq, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method=method)
        assert eng.last_jvp_kernel == kernel, (method, eng.last_jvp_kernel)
        torch.cuda.synchronize()
        out[method] = tuple(t.cpu().numpy() for t in got) + (eng.last_lsqr_iters.cpu().numpy(),)
    return out["direct"], out["lsqr"]


def _errors(d, l):
    """per instance: max over dx, dy, ds of  max |direct - lsqr| / (1 + max |lsqr|)"""
    return np.max([np.abs(d[k] - l[k]).max(axis=1) / (1 + np.abs(l[k]).max(axis=1)) for k in range(3)], axis=0)


def _check_regular_against_lsqr(d, l, min_regular):
    """the reference must itself have converged (status 0) where it is compared; at most 10 % of the batch may be left out for that"""
    ref_ok = l[3] == 0
    assert ref_ok.mean() >= 0.9, ref_ok.mean()
    reg = d[3] == 0
    print("regular share", reg.mean(), "direct status counts", np.bincount(d[3]), "reference not converged", int((~ref_ok).sum()))
    assert reg.mean() >= min_regular, (reg.mean(), np.bincount(d[3]))
    assert (d[4][reg] == 0).all() and (d[4][~reg] > 0).all(), d[4]
    cmp_ = reg & ref_ok
    for k, name in enumerate(("dx", "dy", "ds")):
        e = (np.abs(d[k] - l[k]).max(axis=1) / (1 + np.abs(l[k]).max(axis=1)))[cmp_]
        print(f"{name}: max {e.max():.3e} median {np.median(e):.3e}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, e.max(), np.median(e))
    return reg, ref_ok


SHAPES = {
    "v0_single_wave": (12, {"z": 2, "l": 6, "q": [4, 5]}, 48, 1, 0, 0.8),
    "v0_small": (8, {"z": 4, "l": 6, "q": [4]}, 32, 2, 0, 0.8),
    "ragged_cones": (20, {"z": 3, "l": 10, "q": [3, 7, 2, 5, 1]}, 48, 4, None, 0.8),
    "soc_only": (25, {"z": 0, "l": 0, "q": [6] * 6}, 32, 5, None, 0.8),
    "v1_metric": (P.CONFIGS["M"]["n"], P.CONFIGS["M"]["cones"], 96, 3, 1, 0.95),
    "v2_512_threads": (P.CONFIGS["C3"]["n"], P.CONFIGS["C3"]["cones"], 32, 7, 2, 0.8),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_direct_equals_lsqr_on_regular_instances(shape):
    n, cones, B, seed, variant, min_regular = SHAPES[shape]
    r = _point(n, cones, B, seed)
    v = _lib.lib().ce_adjoint_ns_variant(r["eng"]._h)
    assert v >= 0 and (variant is None or v == variant), v
    d, l = _both(r)
    _check_regular_against_lsqr(d, l, min_regular)


def _assert_transpose_identity_direct(r, seed, method):
    """test_gpu_jvp.py::_assert_transpose_identity with the JVP's method as an argument:
    <x-bar, dx> + <y-bar, dy>  ==  <dA_eval, tA_eval> + <dq_eval, tq_eval>  per instance, to 1e-6 (1 + |lhs| + |rhs|), on the instances both calls solve directly"""
    eng, (x, y, s) = r["eng"], r["pt"]
    rng = np.random.default_rng(seed)
    xb = torch.from_numpy(rng.standard_normal(tuple(x.shape))).cuda(); yb = torch.from_numpy(rng.standard_normal(tuple(y.shape))).cuda()
    dx, dy, ds, st = eng.jvp(r["A_bm"], x, y, s, r["tA_bm"], r["tq"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method=method)
    assert eng.last_jvp_kernel == "ce_jvp"
    dA, dq, adj = eng.vjp(r["A_bm"], x, y, s, xb, yb, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"])
    torch.cuda.synchronize()
    st, adj = st.cpu().numpy(), adj.cpu().numpy()
    assert ((st & 3) == 0).all() and ((adj & 3) == 0).all(), (st, adj)
    assert (st == adj).all(), (st, adj)          # the same elimination flags the same instances
    assert (st == 0).mean() >= 0.8
    lhs = ((xb * dx).sum(dim=1) + (yb * dy).sum(dim=1)).cpu().numpy()
    rhs = ((dA.t() * r["tA_bm"]).sum(dim=1) + (dq * r["tq"]).sum(dim=0)).cpu().numpy()
    print("transpose identity: max |lhs - rhs| / (1 + |lhs| + |rhs|) =", (np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))).max())
    assert (np.abs(lhs - rhs) < 1e-6 * (1 + np.abs(lhs) + np.abs(rhs))).all(), (lhs, rhs)
    assert np.abs(lhs).max() > 1e-3


@pytest.mark.parametrize("n,cones,B,seed", [(P.CONFIGS["M"]["n"], P.CONFIGS["M"]["cones"], 48, 0), (12, {"z": 2, "l": 6, "q": [4, 5]}, 48, 1)])
def test_transpose_identity_of_the_direct_jvp_against_the_search_free_adjoint(n, cones, B, seed):
    _assert_transpose_identity_direct(_point(n, cones, B, seed), seed + 2, "direct")


def test_direct_jvp_is_the_derivative_of_the_gpu_solution_map():
    """recipe and bound of test_gpu_jvp.py::test_jvp_is_the_derivative_of_the_gpu_solution_map (central differences of eng.solve, h = 1e-5)"""
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    n, cones, B = 12, {"z": 2, "l": 10, "q": [4, 5]}, 8
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=7)
    eng = _engine(tpl)
    st = make_settings(dict(acceleration_lookback=0, eps=1e-11, max_iters=200000))

    def solve(A_, b_, c_):
        A_eval, q_eval = tpl.values_from_dense(A_, b_, c_)
        A_bm = torch.from_numpy(A_eval).cuda().t().contiguous(); q_t = torch.from_numpy(q_eval).cuda()
        x, y, s, _, status, _ = eng.solve(A_bm, q_t, st)
        assert (status.cpu().numpy() == 1).all()
        return A_bm, q_t, (x, y, s)
    A_bm, q_t, (x, y, s) = solve(A, b, c)
    (dA, db, dc), tA_bm, tq = _tangents(tpl, B, seed=3)
    got = eng.jvp(A_bm, x, y, s, tA_bm, tq, q_eval=q_t, method="direct")
    assert eng.last_jvp_kernel == "ce_jvp" and ((got[3].cpu().numpy() & 3) == 0).all()
    print("status", got[3].cpu().numpy(), "iters", eng.last_lsqr_iters.cpu().numpy())
    h = 1e-5
    plus = solve(A + h * dA, b + h * db, c + h * dc)[2]; minus = solve(A - h * dA, b - h * db, c - h * dc)[2]
    for name, g, p_, m_ in zip("xys", got[:3], plus, minus):
        fd = ((p_ - m_) / (2 * h)).cpu().numpy(); an = g.cpu().numpy()
        print(f"d{name}: max |jvp - fd| = {np.abs(fd - an).max():.3e}, max |jvp| = {np.abs(an).max():.3e}")
        assert np.abs(fd - an).max() < 2e-4 * (1 + np.abs(an).max()), (name, np.abs(fd - an).max())


def test_duplicated_equality_rows_are_flagged_and_resolved():
    """set-up of test_gpu_ns_adjoint.py::test_duplicated_equality_rows_are_flagged_by_the_row_elimination_and_resolved: every second instance has a redundant
    equality row; the row elimination drops it, flags the instance and the LSQR launch behind the kernel re-solves it -- the same kernel, rule and start as the
    LSQR call's"""
    def mutate(A, b):
        deg = np.arange(A.shape[0]) % 2 == 0
        A[deg, 2, :] = A[deg, 0, :]; b[deg, 2] = b[deg, 0]
        return deg
    r = _point(12, {"z": 4, "l": 8, "q": [5]}, 24, 11, eps=1e-10, min_solved=0.8, mutate=mutate)
    deg = r["extra"][r["keep"]]
    d, l = _both(r)
    assert (d[3][deg] == 12).all() and (d[3][~deg] == 0).all(), d[3]
    assert (d[4][deg] > 0).all() and (d[4][~deg] == 0).all(), d[4]
    assert (l[3][deg] == 0).all()
    for k, name in enumerate(("dx", "dy", "ds")):
        e = np.abs(d[k][deg] - l[k][deg]).max() / (1 + np.abs(l[k][deg]).max())
        print(name, "re-solved vs lsqr:", e)
        assert e < 1e-6, (name, e)
    ok = ~deg & (l[3] == 0)
    assert ok.sum() >= 0.9 * (~deg).sum()
    e = _errors(d, l)[ok]
    assert e.max() < 1e-5 and np.median(e) < 1e-8, (e.max(), np.median(e))


def test_lp_vertices_are_solved_or_flagged_and_agree_with_lsqr():
    """nonneg-only programs: nf = 0 at a non-degenerate vertex; more active rows than variables is rank deficient by counting and goes to LSQR"""
    r = _point(10, {"z": 0, "l": 30, "q": []}, 64, 9, eps=1e-10)
    d, l = _both(r)
    reg, fl = d[3] == 0, (d[3] & 8) != 0
    print("regular", reg.mean(), "flagged", fl.mean(), "status counts", np.bincount(d[3]))
    assert (reg | fl).all() and reg.mean() > 0.5
    ref_ok = l[3] == 0
    assert ref_ok.mean() >= 0.9
    e = _errors(d, l)
    assert e[reg & ref_ok].max() < 1e-5, e[reg & ref_ok].max()
    if fl.any():
        assert ((d[3][fl] & 3) == 0).all() and (d[4][fl] > 0).all()
        ef = e[fl & ref_ok]
        print("flagged vs lsqr: median", np.median(ef), "max", ef.max())
        assert np.median(ef) < 1e-6 and ef.max() < 5e-3, ef


def test_null_tangents():
    r = _point(12, {"z": 2, "l": 6, "q": [4, 5]}, 16, 1)
    eng = r["eng"]
    dx, dy, ds, st = eng.jvp(r["A_bm"], *r["pt"], None, None, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    assert eng.last_jvp_kernel == "ce_jvp"
    assert (dx == 0).all() and (dy == 0).all() and (ds == 0).all() and (st == 0).all() and (eng.last_lsqr_iters == 0).all()
    a = eng.jvp(r["A_bm"], *r["pt"], None, r["tq"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    b = eng.jvp(r["A_bm"], *r["pt"], torch.zeros_like(r["tA_bm"]), r["tq"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    assert (a[3] == b[3]).all() and (a[0].abs().max() > 0)
    reg = a[3] == 0
    assert reg.float().mean() >= 0.8
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u[reg], v[reg])
        assert torch.allclose(u, v, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("case", ["case_ridge_batched_matrix_param", "case_ridge_unbatched"])
def test_forward_ad_through_the_layer_with_jvp_mode_direct(case):
    from cvxpylayers_amd.torch import CvxpyLayer
    cs = getattr(ref_cases, case)()
    layer = CvxpyLayer(template=cs["template"], solver_args={**ref_cases.SOLVER_ARGS, "jvp_mode": "direct"})
    F0, g0 = (torch.from_numpy(p).cuda() for p in cs["params"])
    gen = torch.Generator(device="cpu").manual_seed(5)
    tF, tg = (torch.randn(t.shape, generator=gen, dtype=torch.float64).cuda() for t in (F0, g0))
    with fwAD.dual_level():
        (xd,) = layer(fwAD.make_dual(F0.clone(), tF), fwAD.make_dual(g0.clone(), tg))
        xt = fwAD.unpack_dual(xd).tangent
        info = layer.info["jvp"]
        print("status", info["status"].cpu().numpy(), "iters", info["iters"].cpu().numpy())
        assert info["path"] == "direct"
        assert (info["status"].cpu().numpy() == 0).all() and (info["iters"].cpu().numpy() == 0).all()
        want = fwAD.unpack_dual(_closed_form(fwAD.make_dual(F0.clone(), tF), fwAD.make_dual(g0.clone(), tg))).tangent
        assert xt is not None and torch.allclose(xt, want, atol=1e-5), (xt - want).abs().max()
        # the default stays LSQR, and says so
        (xl,) = layer(fwAD.make_dual(F0.clone(), tF), fwAD.make_dual(g0.clone(), tg), solver_args={"jvp_mode": "lsqr"})
        assert layer.info["jvp"]["path"] == "lsqr" and (layer.info["jvp"]["iters"].cpu().numpy() > 0).all()
        assert torch.allclose(fwAD.unpack_dual(xl).tangent, want, atol=1e-5)


def test_jvp_mode_direct_falls_back_to_lsqr_on_a_psd_template_and_says_so():
    from cvxpylayers_amd.torch import CvxpyLayer
    cs = ref_cases.case_sdp_symmetric_primal_and_psd_dual()
    (C0,) = (torch.from_numpy(p).cuda() for p in cs["params"])
    gen = torch.Generator(device="cpu").manual_seed(6)
    tC = torch.randn(C0.shape, generator=gen, dtype=torch.float64).cuda()
    got = {}
    for mode in ("direct", "lsqr"):
        layer = CvxpyLayer(template=cs["template"], solver_args={**ref_cases.SOLVER_ARGS, "jvp_mode": mode})
        with fwAD.dual_level():
            outs = layer(fwAD.make_dual(C0.clone(), tC))
            got[mode] = [fwAD.unpack_dual(o).tangent.clone() for o in outs]
            assert layer.info["jvp"]["path"] == "lsqr" and (layer.info["jvp"]["iters"].cpu().numpy() > 0).all()
    for a, b in zip(got["direct"], got["lsqr"]):
        assert torch.equal(a, b)
    # the library's own refusal (per-instance path of a PSD template): ConeEngine.jvp runs the LSQR entry point and records it
    r = _point(4, {"z": 1, "s": [3]}, 5, 6, eps=1e-10)
    eng = r["eng"]
    assert _lib.lib().ce_adjoint_ns_variant(eng._h) < 0
    d = eng.jvp(r["A_bm"], *r["pt"], r["tA_bm"], r["tq"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    assert eng.last_jvp_kernel == "ce_jvp_lsqr" and (eng.last_lsqr_iters > 0).all()
    l = eng.jvp(r["A_bm"], *r["pt"], r["tA_bm"], r["tq"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="lsqr")
    assert all(torch.equal(u, v) for u, v in zip(d, l))


def test_unknown_jvp_mode_is_an_error():
    from cvxpylayers_amd.torch import CvxpyLayer
    cs = ref_cases.case_ridge_unbatched()
    layer = CvxpyLayer(template=cs["template"], solver_args={**ref_cases.SOLVER_ARGS, "jvp_mode": "nonsense"})
    F0, g0 = (torch.from_numpy(p).cuda() for p in cs["params"])
    with pytest.raises(ValueError, match="jvp_mode"):
        layer(F0, g0)
    r = _point(8, {"z": 4, "l": 6, "q": [4]}, 4, 2)
    with pytest.raises(ValueError, match="method"):
        r["eng"].jvp(r["A_bm"], *r["pt"], r["tA_bm"], r["tq"], q_eval=r["q_t"], method="nonsense")

"""Forward-mode derivative of the layer (diffcp's `derivative`, D): k_sa_lsqr<..., FWD> behind ce_jvp_lsqr / ce_jvp_shared_a, ConeEngine.jvp, _ConeLayer.jvp and the
frontend's jvp methods.  The reference plugin never calls diffcp's forward derivative, so the checks are
  * finite differences of the GPU solve itself (the derivative of the solution map),
  * the transpose identity  <x-bar, dx> + <y-bar, dy> = <dA_eval, tA_eval> + <dq_eval, tq_eval>  against the adjoint kernel the oracle pins (exact for
    pseudo-inverses: it also holds on rank-deficient systems), on every cone type and on the shared-A split products,
  * a dense known answer built in numpy at the oracle's point,
  * torch.autograd.forward_ad through cvxpylayers_amd.torch.CvxpyLayer against forward-mode AD of the closed form."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import ref_cases
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR

pytestmark = pytest.mark.gpu


def _engine(tpl):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    return ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))


def _at_oracle_point(tpl, A, b, c, eps, max_iters=200000):
    """engine, batch-major values, q_eval and the oracle's (x, y, s) on the device"""
    from oracle import oracle
    ref = oracle.solve_batch(A, b, c, tpl.cones, eps=eps, max_iters=max_iters)
    assert (ref["status"] == 1).all()
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = _engine(tpl)
    A_bm = torch.from_numpy(A_eval).cuda().t().contiguous()
    return eng, A_bm, torch.from_numpy(q_eval).cuda(), tuple(torch.from_numpy(ref[k]).cuda() for k in ("x", "y", "s")), ref


def _tangents(tpl, B, seed, with_A=True):
    """random solver-form tangents (dA, db, dc) as boundary tangents tA_bm (B, nnz_aug), tq (n+1, B): the value maps are linear"""
    rng = np.random.default_rng(seed)
    dA = rng.standard_normal((B, tpl.m, tpl.n)) if with_A else np.zeros((B, tpl.m, tpl.n))
    db = rng.standard_normal((B, tpl.m)); dc = rng.standard_normal((B, tpl.n))
    tA_eval, tq_eval = tpl.values_from_dense(dA, db, dc)
    return (dA, db, dc), torch.from_numpy(tA_eval).cuda().t().contiguous(), torch.from_numpy(tq_eval).cuda()


def _assert_transpose_identity(eng, A_bm, q_t, pt, tA_bm, tq, seed, vjp_path, jvp_path, rule=TIGHT_LSQR):
    """<x-bar, dx> + <y-bar, dy>  ==  <dA_eval, tA_eval> + <dq_eval, tq_eval>  per instance, to 1e-6 (1 + |lhs| + |rhs|)"""
    x, y, s = pt
    rng = np.random.default_rng(seed)
    xb = torch.from_numpy(rng.standard_normal(tuple(x.shape))).cuda(); yb = torch.from_numpy(rng.standard_normal(tuple(y.shape))).cuda()
    dx, dy, ds, st = eng.jvp(A_bm, x, y, s, tA_bm, tq, path=jvp_path, lsqr=rule, q_eval=q_t)
    dA, dq, adj = eng.vjp(A_bm, x, y, s, xb, yb, path=vjp_path, lsqr=rule, q_eval=q_t)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and (adj.cpu().numpy() == 0).all()
    lhs = ((xb * dx).sum(dim=1) + (yb * dy).sum(dim=1)).cpu().numpy()
    rhs = ((dA.t() * tA_bm).sum(dim=1) + (dq * tq).sum(dim=0)).cpu().numpy()
    print("transpose identity: max |lhs - rhs| / (1 + |lhs| + |rhs|) =", (np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))).max())
    assert (np.abs(lhs - rhs) < 1e-6 * (1 + np.abs(lhs) + np.abs(rhs))).all(), (lhs, rhs)
    assert np.abs(lhs).max() > 1e-3          # (the identity is not 0 = 0)
    return dx, dy, ds


def test_jvp_is_the_derivative_of_the_gpu_solution_map():
    """central differences of eng.solve itself (h = 1e-5) in x, y and s, all of A, b, c perturbed at once; bound and recipe of
    test_gpu_fullsize.py::test_adjoint_is_the_derivative_of_the_gpu_solution_map"""
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
    got = eng.jvp(A_bm, x, y, s, tA_bm, tq, q_eval=q_t)
    assert (got[3].cpu().numpy() == 0).all()
    h = 1e-5
    plus = solve(A + h * dA, b + h * db, c + h * dc)[2]; minus = solve(A - h * dA, b - h * db, c - h * dc)[2]
    for name, g, p_, m_ in zip("xys", got[:3], plus, minus):
        fd = ((p_ - m_) / (2 * h)).cpu().numpy(); an = g.cpu().numpy()
        print(f"d{name}: max |jvp - fd| = {np.abs(fd - an).max():.3e}, max |jvp| = {np.abs(an).max():.3e}")
        assert np.abs(fd - an).max() < 2e-4 * (1 + np.abs(an).max()), (name, np.abs(fd - an).max())


def test_transpose_identity_against_the_pinned_adjoint_at_the_metric_shape():
    cfg = P.CONFIGS["M"]; n, cones, B = cfg["n"], cfg["cones"], 48
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=0)
    eng, A_bm, q_t, pt, _ = _at_oracle_point(tpl, A, b, c, 1e-9)
    _, tA_bm, tq = _tangents(tpl, B, seed=1)
    _assert_transpose_identity(eng, A_bm, q_t, pt, tA_bm, tq, 2, "per_instance_lsqr", "per_instance")
    # diffcp's default rule (1e-8 / 1e-8 / 2 N): the kernel iterates, and stops before the limit
    *_, st = eng.jvp(A_bm, *pt, tA_bm, tq, path="per_instance", q_eval=q_t)
    its = eng.last_lsqr_iters.cpu().numpy()
    assert (st.cpu().numpy() == 0).all() and (its > 0).all() and (its < 2 * (tpl.n + tpl.m + 1)).all(), its


def test_dense_known_answer_without_the_adjoint():
    """M built densely in numpy at the oracle's eps = 1e-12 point (plain cones: DPi is the 0/1 diagonal y - s > 0, 1 on zero-cone rows), d = lstsq(M, -dQ pi)"""
    n, cones, B = 6, {"z": 2, "l": 10}, 4
    tpl = P.dense_template(n, cones); m = tpl.m
    A, b, c = P.generate(n, cones, B, seed=4)
    eng, A_bm, q_t, pt, ref = _at_oracle_point(tpl, A, b, c, 1e-12)
    (dA, db, dc), tA_bm, tq = _tangents(tpl, B, seed=5)
    dx, dy, ds, st = eng.jvp(A_bm, *pt, tA_bm, tq, path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t)
    assert (st.cpu().numpy() == 0).all()
    for i in range(B):
        x, y, s = ref["x"][i], ref["y"][i], ref["s"][i]
        D = np.diag(np.concatenate([np.ones(cones["z"]), (y - s > 0)[cones["z"]:].astype(float)]))
        M = np.zeros((n + m + 1, n + m + 1))
        M[:n, n:n + m] = A[i].T @ D; M[:n, -1] = c[i]
        M[n:n + m, :n] = -A[i]; M[n:n + m, n:n + m] = np.eye(m) - D; M[n:n + m, -1] = b[i]
        M[-1, :n] = -c[i]; M[-1, n:n + m] = -b[i] @ D
        g = np.concatenate([dA[i].T @ y + dc[i], -dA[i] @ x + db[i], [-(dc[i] @ x) - db[i] @ y]])
        d = np.linalg.lstsq(M, -g, rcond=None)[0]
        q = D @ d[n:n + m]
        want = (d[:n] - x * d[-1], q - y * d[-1], q - d[n:n + m] - s * d[-1])
        for name, got, w in zip(("dx", "dy", "ds"), (dx, dy, ds), want):
            err = np.abs(got[i].cpu().numpy() - w).max()
            assert err < 1e-6 * (1 + np.abs(w).max()), (i, name, err)


@pytest.mark.parametrize("name,n,cones", [("psd", 4, {"z": 1, "s": [3]}), ("exp", 5, {"l": 4, "ep": 2}), ("pow", 5, {"l": 4, "p": [0.4]})])
def test_transpose_identity_on_every_cone_type(name, n, cones):
    B = 5
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=6)
    eng, A_bm, q_t, pt, _ = _at_oracle_point(tpl, A, b, c, 1e-10)
    _, tA_bm, tq = _tangents(tpl, B, seed=7)
    _assert_transpose_identity(eng, A_bm, q_t, pt, tA_bm, tq, 8, "per_instance_lsqr", "per_instance")


def test_transpose_identity_on_a_shared_A_template_through_the_split_products(monkeypatch):
    """ce_jvp_shared_a (RP > 0: singleton / dense-row split), tangents in b and c only"""
    B = 6
    A, b, c, cones, tpl = P.portfolio_c5_batch(B, seed=3, nw=60, kf=9)
    Ab = np.broadcast_to(A, (B,) + A.shape).copy(); bb = np.broadcast_to(b, (B,) + b.shape).copy()
    monkeypatch.setenv("CE_CONST_A", "1")
    eng, A_bm, q_t, pt, _ = _at_oracle_point(tpl, Ab, bb, c, 1e-8)
    _, tA_bm, tq = _tangents(tpl, B, seed=9, with_A=False)
    _assert_transpose_identity(eng, A_bm, q_t, pt, tA_bm, tq, 10, "const_a", "const_a")
    assert eng.last_jvp_kernel == "ce_jvp_shared_a" and eng.plan()["sp_RP"] > 0


def test_transpose_identity_on_a_rank_deficient_system():
    """a duplicated equality row (the set-up of test_gpu_lsqr_mode.py's minimum-norm test): M is rank deficient beyond its homogeneity direction; the identity is
    exact for pseudo-inverses, so it holds between the two minimum-norm solutions.  Both LSQR runs converge under the default conlim = 1e8 here (status 0)."""
    n, cones, B = 8, {"z": 4, "l": 6, "q": [4]}, 6
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=2)
    A[:, 1, :] = A[:, 0, :]; b[:, 1] = b[:, 0]
    eng, A_bm, q_t, pt, _ = _at_oracle_point(tpl, A, b, c, 1e-10)
    _, tA_bm, tq = _tangents(tpl, B, seed=11)
    _assert_transpose_identity(eng, A_bm, q_t, pt, tA_bm, tq, 12, "per_instance_lsqr", "per_instance")


def _closed_form(F, g):
    n = F.shape[-1]
    eye = torch.eye(n, dtype=F.dtype, device=F.device)
    return torch.linalg.solve(F.transpose(-1, -2) @ F + eye, (F.transpose(-1, -2) @ g.unsqueeze(-1))).squeeze(-1)


@pytest.mark.parametrize("case", ["case_ridge_batched_matrix_param", "case_ridge_unbatched"])
def test_forward_ad_through_the_layer_matches_the_closed_form(case):
    from cvxpylayers_amd.torch import CvxpyLayer
    cs = getattr(ref_cases, case)()
    layer = CvxpyLayer(template=cs["template"], solver_args=ref_cases.SOLVER_ARGS)
    F0, g0 = (torch.from_numpy(p).cuda() for p in cs["params"])
    w = torch.from_numpy(cs["weights"][0]).cuda()
    gen = torch.Generator(device="cpu").manual_seed(5)
    tF, tg = (torch.randn(t.shape, generator=gen, dtype=torch.float64).cuda() for t in (F0, g0))

    def plain():
        F, g = F0.clone().requires_grad_(), g0.clone().requires_grad_()
        (x,) = layer(F, g)
        (x * w).sum().backward()
        return x.detach().clone(), F.grad.clone(), g.grad.clone()
    x_ref, gF_ref, gg_ref = plain()
    with fwAD.dual_level():
        F, g = F0.clone().requires_grad_(), g0.clone().requires_grad_()
        (xd,) = layer(fwAD.make_dual(F, tF), fwAD.make_dual(g, tg))
        xp, xt = fwAD.unpack_dual(xd)
        assert xt is not None and xt.shape == xp.shape == x_ref.shape
        info = layer.info["jvp"]
        assert (info["status"].cpu().numpy() == 0).all() and (info["iters"].cpu().numpy() > 0).all()
        want = fwAD.unpack_dual(_closed_form(fwAD.make_dual(F0.clone(), tF), fwAD.make_dual(g0.clone(), tg))).tangent
        assert torch.allclose(xt, want, atol=1e-5), (xt - want).abs().max()
        # the dual level changes nothing else: same primal values, same reverse-mode gradients, bit for bit
        (xp * w).sum().backward()
        assert torch.equal(xp.detach(), x_ref) and torch.equal(F.grad, gF_ref) and torch.equal(g.grad, gg_ref)
        # no_grad (needs_grad False) with dual inputs still returns tangents
        with torch.no_grad():
            (xn,) = layer(fwAD.make_dual(F0.clone(), tF), fwAD.make_dual(g0.clone(), tg))
        xnt = fwAD.unpack_dual(xn).tangent
        assert xnt is not None and torch.allclose(xnt, want, atol=1e-5)
    # outside a dual level: no tangent, nothing recorded for it
    (x_plain,) = layer(F0, g0)
    assert fwAD.unpack_dual(x_plain).tangent is None and torch.equal(x_plain, x_ref)


def test_c_abi_null_tangents_give_zero_outputs():
    n, cones, B = 6, {"z": 2, "l": 10}, 4
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=4)
    eng, A_bm, q_t, (x, y, s), _ = _at_oracle_point(tpl, A, b, c, 1e-9)
    out = [torch.full(sh, 7.0, dtype=torch.float64, device="cuda") for sh in ((B, tpl.n), (B, tpl.m), (B, tpl.m))]
    st = torch.full((B,), -1, dtype=torch.int32, device="cuda"); its = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fn in (_lib.lib().ce_jvp_lsqr, _lib.lib().ce_jvp_shared_a):
        rc = fn(eng._h, B, A_bm.data_ptr(), tpl.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                None, 0, None, 0, 0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), st.data_ptr(), its.data_ptr(), 1e-8, 1e-8, 1e8, 0, stream)
        assert rc == 0, _lib.lib().ce_last_error()
        torch.cuda.synchronize()
        assert all((o == 0).all() for o in out) and (st == 0).all() and (its == 0).all()
        for o in out:
            o.fill_(7.0)
    # ds may be NULL; ConeEngine.jvp with both tangents None is the same call
    rc = _lib.lib().ce_jvp_lsqr(eng._h, B, A_bm.data_ptr(), tpl.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                                None, 0, None, 0, 0, out[0].data_ptr(), out[1].data_ptr(), None, st.data_ptr(), its.data_ptr(), 1e-8, 1e-8, 1e8, 0, stream)
    torch.cuda.synchronize()
    assert rc == 0 and (out[0] == 0).all() and (out[1] == 0).all() and (out[2] == 7.0).all()
    dx, dy, ds, st2 = eng.jvp(A_bm, x, y, s, None, None, path="per_instance", q_eval=q_t)
    assert (dx == 0).all() and (dy == 0).all() and (ds == 0).all() and (st2 == 0).all()


def test_native_quadratic_objective_is_refused_and_points_to_the_epigraph_form():
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    from test_quad_objective import _eq_qp, _upper_structure
    n, p, B = 6, 2, 3
    Pm, q, F, g = _eq_qp(n, p, B, seed=1)
    cones = {"z": p, "l": 0, "q": [], "s": []}
    tpl = P.dense_template(n, cones)
    pst = _upper_structure(n)
    ctx = MI355_ctx(pst, tpl.problem_data_index, cones, options={"eps": 1e-9, "max_iters": 200000})
    dev = torch.device("cuda", 0)
    eng = ctx.engine(dev)
    assert eng.qp_native
    idx, ptr, _ = pst
    pcols = np.repeat(np.arange(n), np.diff(ptr))
    P_eval = torch.from_numpy(np.ascontiguousarray(Pm[:, idx, pcols].T)).to(dev)
    A_eval, q_eval = tpl.values_from_dense(F, g, q)
    A_t, q_t = torch.from_numpy(A_eval).to(dev), torch.from_numpy(q_eval).to(dev)
    # the C ABI
    z = torch.zeros((B, max(tpl.n, tpl.m)), dtype=torch.float64, device=dev); st = torch.zeros((B,), dtype=torch.int32, device=dev)
    A_bm = A_t.t().contiguous()
    rc = _lib.lib().ce_jvp_lsqr(eng._h, B, A_bm.data_ptr(), tpl.nnz_aug, None, 0, 0, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, 0, None, 0, 0,
                                z.data_ptr(), z.data_ptr(), None, st.data_ptr(), None, 1e-8, 1e-8, 1e8, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -2 and b"epigraph" in _lib.lib().ce_last_error()
    # the plugin
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError, match="CE_QP_EPIGRAPH"):
            _CvxpyLayer.apply(P_eval, fwAD.make_dual(q_t, torch.ones_like(q_t)), A_t, ctx, {}, True, None)


def test_plugin_fills_info_and_masks_failed_instances_with_nan_tangents():
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    n, cones, B = 6, {"z": 2, "l": 10}, 4
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=4)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    ctx = MI355_ctx(None, tpl.problem_data_index, cones, options={"eps": 1e-9, "max_iters": 100000})
    A_t, q_t = torch.from_numpy(A_eval).cuda(), torch.from_numpy(q_eval).cuda()
    _, tA_bm, tq = _tangents(tpl, B, seed=5)
    with fwAD.dual_level():
        primal, dual, info, _ = _CvxpyLayer.apply(None, fwAD.make_dual(q_t, tq), fwAD.make_dual(A_t, tA_bm.t()), ctx, {}, False, None)      # needs_grad=False: still tangents
        tp, td = fwAD.unpack_dual(primal).tangent, fwAD.unpack_dual(dual).tangent
        assert tp.shape == (B, n) and td.shape == (B, tpl.m) and torch.isfinite(tp).all()
        assert info["jvp"]["status"].shape == (B,) and (info["jvp"]["iters"].cpu().numpy() > 0).all()
        eng = ctx.engine(torch.device("cuda", 0))
        assert eng.last_jvp_kernel == "ce_jvp_lsqr"
        # raise_on_error=False with an infeasible instance (a nonnegative row  0 x + s = -1): NaN primal and NaN tangent there, the other instances as before
        A2, b2 = A.copy(), b.copy()
        A2[0, 2, :] = 0.0; b2[0, 2] = -1.0
        A_eval2, _ = tpl.values_from_dense(A2, b2, c)
        primal2, _, info2, _ = _CvxpyLayer.apply(None, fwAD.make_dual(q_t, tq), fwAD.make_dual(torch.from_numpy(A_eval2).cuda(), tA_bm.t()), ctx, {"raise_on_error": False}, True, None)
        pp2, tp2 = fwAD.unpack_dual(primal2)
        assert (info2["status"].cpu().numpy()[0] < 0) and torch.isnan(pp2[0]).all() and torch.isnan(tp2[0]).all()
        assert torch.isfinite(tp2[1:]).all() and torch.allclose(tp2[1:], tp[1:], rtol=1e-6, atol=1e-9)

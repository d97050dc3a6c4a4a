"""K cotangents at one solution of a template with PSD blocks on one factorisation per instance: k_backward_ns<..., MANY, PSD> (no FWD) behind ce_vjp_psd_many,
ConeEngine.vjp_many(psd_many=True).

Shapes are psd_ns_kit.SHAPES, all five, at the oracle's points (eps 1e-10, every instance Solved); K and the cotangent pattern are test_gpu_vjp_many's: K in
(1, 3, 17), cotangent 0 repeated at K - 1, an all-zero cotangent at position 1 (psd_many_kit).  Checked against
  * the dense transposed system of psd_many_kit (D from psd_ns_kit.proj, J^T r = (dx; D dy), mapped by test_gpu_ns_adjoint._boundary): 1e-5 worst, 1e-8 median
    relative to 1 + max |reference| on every instance with status 0, which must be >= 80 % for every k;
  * the same engine's loop of K pivoting ce_vjp calls (force_loop=True): 1e-6 where both routes report status 0 (>= 80 %), flags equal across k, the repeat
    bit-identical, the zero cotangent exact zeros;
  * the transpose identity against ce_jvp_psd;
  * a duplicated equality row and the planted stiff block: 12 for every k, re-solved in one launch -- values torch.equal to K single ce_vjp_lsqr calls under
    TIGHT_LSQR, whose status is 0 (the adjoint entry points return no iteration counts for a listed instance: the forward file pins those);
  * the defaults and refusals that stay."""
import numpy as np
import pytest
import torch

import psd_many_kit as M
import psd_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_jvp import _engine

pytestmark = pytest.mark.gpu
VKW = dict(path="per_instance", lsqr=TIGHT_LSQR)


@pytest.mark.parametrize("Kc", M.KS)
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_every_cotangent_against_the_dense_reference(name, Kc):
    """fails on a tree without the mode: vjp_many takes no psd_many there"""
    r = M.point(name)
    L = _lib.lib()
    want_plan = K.host_plan(*K.SHAPES[name][:2])
    assert L.ce_vjp_psd_many_variant(r["eng"]._h) == want_plan["psd_ns_variant"] == L.ce_psd_ns_variant(r["eng"]._h) >= 0
    assert L.ce_vjp_many_variant(r["eng"]._h) == -1 and L.ce_vjp_tri_many_variant(r["eng"]._h) == -1 and L.ce_adjoint_ns_variant(r["eng"]._h) == -1
    M.check_vjp_against_dense(r, Kc)


@pytest.mark.parametrize("Kc", M.KS)
@pytest.mark.parametrize("name", ["psd_mixed", "lqr_like", "row2_n80"])
def test_every_cotangent_against_the_loop_of_pivoting_calls(name, Kc):
    r = M.point(name)
    o, l = M.run_vjp(r, Kc), M.run_vjp(r, Kc, loop=True)
    assert o["kernel"] == "ce_vjp_psd_many" and l["path"] == "loop" and l["kernel"] is None
    (dA, dq, adj), (dA_l, dq_l, adj_l) = o["out"], l["out"]
    assert ((adj & 12) == (adj[:1] & 12)).all()          # flags are the matrix's: the same for every cotangent
    both = (adj == 0) & (adj_l == 0)
    assert (both.double().mean(dim=1) >= M.MIN_SHARE).all(), (name, Kc, both.double().mean(dim=1))
    eA = ((dA - dA_l).abs().amax(dim=2) / (1 + dA_l.abs().amax(dim=2)))[both]
    eq = ((dq - dq_l).abs().amax(dim=2) / (1 + dq_l.abs().amax(dim=2)))[both]
    print(f"{name} K={Kc}: against the loop dA {eA.max().item():.2e} dq {eq.max().item():.2e}; flagged here {int((adj[0] != 0).sum())}, by the pivoting kernel {int((adj_l[0] != 0).sum())}")
    assert eA.max().item() < 1e-6 and eq.max().item() < 1e-6, (name, Kc, eA.max().item(), eq.max().item())
    if Kc >= 3:
        un = adj[M.ZERO_AT] == 0
        assert (dA[M.ZERO_AT][un] == 0).all() and (dq[M.ZERO_AT][un] == 0).all()
        assert torch.equal(dA[0], dA[Kc - 1]) and torch.equal(dq[0], dq[Kc - 1]) and torch.equal(adj[0], adj[Kc - 1])          # the repeated cotangent, first and last


@pytest.mark.parametrize("name", ["psd_mixed", "lqr_like"])
def test_transpose_identity_against_the_forward_derivative(name):
    """<x-bar_k, dx> + <y-bar_k, dy>  ==  <dA_k, tA_eval> + <dq_k, tq_eval>  per instance and cotangent, against ce_jvp_psd (the single-tangent PSD mode)"""
    r = M.point(name)
    eng, (x, y, s) = r["eng"], r["pt"]
    Kc = 3
    tA_bm, tq = torch.from_numpy(r["base_tA"][0]).cuda(), torch.from_numpy(r["base_tq"][0]).cuda().t()
    dx, dy, ds, st = eng.jvp(r["A_bm"], x, y, s, tA_bm, tq, q_eval=r["q_t"], method="direct", psd_ns=True, **VKW)
    assert eng.last_jvp_kernel == "ce_jvp_psd"
    torch.cuda.synchronize()
    dA, dq, adj = (t.cpu().numpy() for t in M.run_vjp(r, Kc)["out"])
    xb, yb = M.pattern(Kc, r["base_dx"], r["base_dy"])
    st = st.cpu().numpy(); dx, dy, tA, tqn = dx.cpu().numpy(), dy.cpu().numpy(), tA_bm.cpu().numpy(), tq.cpu().numpy().T
    for k in (0, 2):
        both = (st == 0) & (adj[k] == 0)
        assert both.mean() >= M.MIN_SHARE, (name, k, both.mean())
        lhs = ((xb[k] * dx).sum(axis=1) + (yb[k] * dy).sum(axis=1))[both]
        rhs = ((dA[k] * tA).sum(axis=1) + (dq[k] * tqn).sum(axis=1))[both]
        print(f"{name} k={k}: transpose identity max |lhs - rhs| / (1 + |lhs| + |rhs|) = {(np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))).max():.2e}, compared {both.mean():.3f}")
        assert (np.abs(lhs - rhs) < 1e-6 * (1 + np.abs(lhs) + np.abs(rhs))).all(), (lhs, rhs)
        assert np.abs(lhs).max() > 1e-3


def _flagged_equal_single_lsqr(eng, A_bm, pt, q_t, dx, dy, out, fl):
    """the flagged instances `fl` of a vjp_many result: status 12 for every k, values bit for bit those of K single ce_vjp_lsqr calls (status 0 there)"""
    dA, dq, adj = out
    assert (adj[:, fl] == 12).all() and (adj[:, ~fl] == 0).all(), adj
    for k in range(dx.shape[0]):
        a1, q1, s1 = eng.vjp(A_bm, *pt, dx[k], dy[k], path="per_instance_lsqr", lsqr=TIGHT_LSQR, q_eval=q_t)
        assert (s1[fl] == 0).all(), s1
        assert torch.equal(dA[k][fl], a1.t()[fl]) and torch.equal(dq[k][fl], q1.t()[fl]), k


def test_duplicated_equality_rows_are_flagged_for_every_cotangent_and_resolved_in_one_launch():
    """psd_mixed with its second equality row a copy of the first on every second instance (test_gpu_psd_jvp.py's construction), K = 3"""
    from oracle import oracle
    n, cones, B, seed = K.SHAPES["psd_mixed"]
    Kc = 3
    A, b, c = P.generate(n, cones, B, seed=seed)
    deg = np.arange(B) % 2 == 0
    A[deg, 1, :] = A[deg, 0, :]; b[deg, 1] = b[deg, 0]
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)
    keep = ref["status"] == 1
    assert keep.mean() >= 0.8, keep.mean()
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A[keep], b[keep], c[keep])
    eng = _engine(tpl)
    A_bm, q_t = torch.from_numpy(A_eval).cuda().t().contiguous(), torch.from_numpy(q_eval).cuda()
    pt = tuple(torch.from_numpy(ref[k][keep]).cuda() for k in "xys")
    rng = np.random.default_rng(seed + 12)
    dx = torch.from_numpy(rng.standard_normal((Kc,) + tuple(pt[0].shape))).cuda(); dy = torch.from_numpy(rng.standard_normal((Kc,) + tuple(pt[1].shape))).cuda()
    out = eng.vjp_many(A_bm, *pt, dx, dy, q_eval=q_t, psd_many=True, **VKW)
    assert eng.last_vjp_many_path == "many" and eng.last_vjp_kernel == "ce_vjp_psd_many"
    print("duplicated rows: status", out[2].cpu().numpy().tolist())
    _flagged_equal_single_lsqr(eng, A_bm, pt, q_t, dx, dy, out, torch.from_numpy(deg[keep]).cuda())


def test_a_planted_stiff_block_is_flagged_for_every_cotangent_and_resolved_in_one_launch():
    """instance 3 of psd_mixed with its first block replaced by U diag(1, 1, -3e-7) U^T (psd_ns_kit.plant_stiff_block): 1 - B = 3e-7 < NS_TRI_STIFF, the threshold
    carried over.  The other instances keep their direct answers bit for bit."""
    r = M.point("psd_mixed")
    eng, inst, Kc = r["eng"], 3, 3
    y, s = K.plant_stiff_block(r["ref"]["y"], r["ref"]["s"], r["cones"], inst)
    assert K.block_states(y[inst] - s[inst], r["cones"])[1] < 1e-5
    pt = (r["pt"][0], torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda())
    base = M.run_vjp(r, Kc)
    out = eng.vjp_many(r["A_bm"], *pt, base["dx"], base["dy"], q_eval=r["q_t"], psd_many=True, **VKW)
    assert eng.last_vjp_kernel == "ce_vjp_psd_many"
    fl = base["out"][2][0] != 0          # (whatever the elimination flags at the unchanged point stays flagged: none on the MI355X)
    assert not fl[inst] and fl.double().mean().item() <= 1 - M.MIN_SHARE
    fl[inst] = True
    _flagged_equal_single_lsqr(eng, r["A_bm"], pt, r["q_t"], base["dx"], base["dy"], out, fl)
    assert all(torch.equal(u[:, ~fl], v[:, ~fl]) for u, v in zip(out, base["out"]))


def test_without_the_flag_the_same_engine_runs_the_loop_bit_for_bit():
    r = M.point("psd_mixed")
    eng, Kc = r["eng"], 3
    dxt, dyt = (torch.from_numpy(a).cuda() for a in M.pattern(Kc, r["base_dx"], r["base_dy"]))
    dA, dq, adj = eng.vjp_many(r["A_bm"], *r["pt"], dxt, dyt, q_eval=r["q_t"], **VKW)
    assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None
    for k in range(Kc):
        a1, q1, s1 = eng.vjp(r["A_bm"], *r["pt"], dxt[k], dyt[k], q_eval=r["q_t"], **VKW)
        assert torch.equal(dA[k], a1.t()) and torch.equal(dq[k], q1.t()) and torch.equal(adj[k], s1)
    # and with the flag where the elimination does not run: no q_eval (no re-solve), force_loop -- the loop, as without it
    for kw in (dict(path="per_instance"), dict(VKW, q_eval=r["q_t"], force_loop=True)):
        got = eng.vjp_many(r["A_bm"], *r["pt"], dxt, dyt, psd_many=True, **kw)
        assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None, kw
        ref = eng.vjp_many(r["A_bm"], *r["pt"], dxt, dyt, **kw)
        assert all(torch.equal(u, v) for u, v in zip(got, ref)), kw


def _same_with_and_without(eng, args, **kw):
    a = eng.vjp_many(*args, psd_many=True, **kw)
    pa = (eng.last_vjp_many_path, eng.last_vjp_kernel)
    b = eng.vjp_many(*args, **kw)
    assert pa == (eng.last_vjp_many_path, eng.last_vjp_kernel), pa
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    return pa


def test_the_flag_changes_nothing_on_templates_without_blocks():
    import tri_ns_kit as T
    from test_gpu_parity import gpu_solve
    rng = np.random.default_rng(5)
    Kc = 2
    # plain cones: ce_vjp_many's one call, as without the flag; raw ce_vjp_psd_many on it: CE_E_UNSUPPORTED, the reason named, nothing written
    n, cones, B = 8, {"z": 2, "l": 6, "q": [4]}, 8
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=1)
    eng, A_bm, x, y, s, *_ = gpu_solve(tpl, A, b, c, eps=1e-9, max_iters=200000)
    q_t = torch.from_numpy(tpl.values_from_dense(A, b, c)[1]).cuda()
    dx = torch.from_numpy(rng.standard_normal((Kc, B, n))).cuda(); dy = torch.from_numpy(rng.standard_normal((Kc, B, tpl.m))).cuda()
    L = _lib.lib()
    assert L.ce_vjp_psd_many_variant(eng._h) == -1
    assert _same_with_and_without(eng, (A_bm, x, y, s, dx, dy), q_eval=q_t, **VKW) == ("many", "ce_vjp_many")
    f64 = dict(dtype=torch.float64, device="cuda")
    dA = torch.full((Kc, B, eng.nnz_aug), 7.0, **f64); dq = torch.full((Kc, B, n + 1), 7.0, **f64)
    A_c = A_bm.contiguous()
    rc = L.ce_vjp_psd_many(eng._h, B, Kc, A_c.data_ptr(), eng.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                           dx.data_ptr(), None, dA.data_ptr(), dq.data_ptr(), None, None)
    msg = (L.ce_last_error() or b"").decode()
    torch.cuda.synchronize()
    assert rc == -2 and "ce_vjp_psd_many" in msg and "no PSD block" in msg, (rc, msg)
    assert (dA == 7.0).all() and (dq == 7.0).all()
    # a template with triples: the loop of pivoting calls, as without the flag
    n, cones, B, seed, _ = T.SHAPES["exp_small"]
    _, _, A, b, c, ref = T.problem("exp_small")
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = _engine(tpl)
    pt = tuple(torch.from_numpy(ref[k]).cuda() for k in "xys")
    dx = torch.from_numpy(rng.standard_normal((Kc, B, n))).cuda(); dy = torch.from_numpy(rng.standard_normal((Kc, B, tpl.m))).cuda()
    assert L.ce_vjp_psd_many_variant(eng._h) == -1
    assert _same_with_and_without(eng, (torch.from_numpy(A_eval).cuda().t().contiguous(), *pt, dx, dy), q_eval=torch.from_numpy(q_eval).cuda(), **VKW) == ("loop", None)
    # and the siblings keep refusing a PSD handle, with their messages
    r = M.point("psd_small")
    e, Bp = r["eng"], r["A"].shape[0]
    dxp = torch.zeros((1, Bp, r["n"]), **f64); dAp = torch.full((1, Bp, e.nnz_aug), 7.0, **f64); dqp = torch.full((1, Bp, r["n"] + 1), 7.0, **f64)
    for fn, frag in ((L.ce_vjp_many, "no many-cotangent elimination"), (L.ce_vjp_tri_many, "no search-free elimination with triples")):
        rc = fn(e._h, Bp, 1, r["A_bm"].data_ptr(), e.nnz_aug, r["q_t"].data_ptr(), r["q_t"].stride(0), r["q_t"].stride(1), *(t.data_ptr() for t in r["pt"]),
                dxp.data_ptr(), None, dAp.data_ptr(), dqp.data_ptr(), None, None)
        assert rc == -2 and frag in (L.ce_last_error() or b"").decode(), (rc, L.ce_last_error())
    torch.cuda.synchronize()
    assert (dAp == 7.0).all() and (dqp == 7.0).all()


def test_the_flag_changes_nothing_on_a_native_quadratic_objective():
    import qp_ns_kit as Q
    from test_quad_objective import _upper_structure
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    n, cones, A, b, c, Pm = Q.instance("small_mixed")
    tpl = P.dense_template(n, cones)
    struct = _upper_structure(n)
    eng = Q.qp_engine(tpl, struct)
    assert eng.qp_native and _lib.lib().ce_vjp_psd_many_variant(eng._h) == -1
    A_bm, q_t, P_bm = Q.device_values(tpl, A, b, c, Pm, struct)
    x, y, s, *_ = eng.solve(A_bm, q_t, make_settings(dict(eps=1e-9, max_iters=200000, acceleration_lookback=0)), P_bm=P_bm)
    B, Kc = A.shape[0], 2
    rng = np.random.default_rng(3)
    dx = torch.from_numpy(rng.standard_normal((Kc, B, n))).cuda(); dy = torch.from_numpy(rng.standard_normal((Kc, B, tpl.m))).cuda()
    assert _same_with_and_without(eng, (A_bm, x, y, s, dx, dy), path="per_instance", q_eval=q_t, P_bm=P_bm) == ("loop", None)


def test_a_null_dy_is_the_zero_cotangent():
    r = M.point("psd_small")
    eng = r["eng"]
    dx, dy = M.pattern(3, r["base_dx"], r["base_dy"])
    dxt = torch.from_numpy(dx).cuda()
    a = eng.vjp_many(r["A_bm"], *r["pt"], dxt, None, q_eval=r["q_t"], psd_many=True, **VKW)
    assert eng.last_vjp_kernel == "ce_vjp_psd_many"
    b = eng.vjp_many(r["A_bm"], *r["pt"], dxt, torch.zeros(dy.shape, dtype=torch.float64, device="cuda"), q_eval=r["q_t"], psd_many=True, **VKW)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and a[0].abs().max() > 0


def test_empty_batches_and_no_cotangent_return_empty_tensors():
    r = M.point("psd_small")
    eng, B, n, m = r["eng"], r["A"].shape[0], r["n"], r["tpl"].m
    z = torch.zeros((0, B, n), dtype=torch.float64, device="cuda")
    dA, dq, adj = eng.vjp_many(r["A_bm"], *r["pt"], z, None, path="per_instance", q_eval=r["q_t"], psd_many=True)
    assert dA.shape == (0, B, eng.nnz_aug) and dq.shape == (0, B, n + 1) and adj.shape == (0, B)
    e = torch.zeros((0, m), dtype=torch.float64, device="cuda")
    dA, dq, adj = eng.vjp_many(r["A_bm"][:0], e[:, :n], e, e, torch.zeros((2, 0, n), dtype=torch.float64, device="cuda"), None, path="per_instance", q_eval=r["q_t"][:, :0],
                               psd_many=True)
    assert dA.shape == (2, 0, eng.nnz_aug) and dq.shape == (2, 0, n + 1) and adj.shape == (2, 0)

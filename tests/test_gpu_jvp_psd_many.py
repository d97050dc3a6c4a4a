"""K tangents at one solution of a template with PSD blocks on one factorisation per instance: k_backward_ns<..., FWD, ..., MANY, PSD> behind ce_jvp_psd_many,
ConeEngine.jvp_many(psd_many=True).

Shapes are psd_ns_kit.SHAPES, all five, at the oracle's points (eps 1e-10, every instance Solved).  K is (1, 3, 17); tangent 1 is all zeros and tangent 0 is
repeated at K - 1 (psd_many_kit).  Checked against
  * psd_ns_kit.dense_jvp on status-0 instances: 1e-5 worst, 1e-8 median relative to 1 + max |reference| -- the bounds test_gpu_psd_jvp.py holds ce_jvp_psd to --, no
    iteration there, status 0 on >= 80 % for every k;
  * the loop of K ce_jvp_psd calls (force_loop=True with the flag): status and iterations equal everywhere, values within 1e-6 on status-0 instances, torch.equal
    on flagged ones;
  * the zero tangent (exact zeros), the repeat (bit-identical), batch-shared tangents against their expansion (bit-identical);
  * the K x K transpose identity with vjp_many(psd_many=True);
  * a duplicated equality row and the planted stiff block: 12 for every k, listed once, re-solved in one launch -- values, status and LSQR iteration counts of the
    flagged pairs torch.equal to K single ce_jvp_psd calls, whose own re-solve is the same LSQR kernel under TIGHT_LSQR, and within 1e-6 of ce_jvp_lsqr;
  * the defaults and refusals that stay."""
import numpy as np
import pytest
import torch

import psd_many_kit as M
import psd_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_jvp import _engine, _tangents

pytestmark = pytest.mark.gpu
KW = dict(path="per_instance", lsqr=TIGHT_LSQR, method="direct")


@pytest.mark.parametrize("Kc", M.KS)
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_every_tangent_against_the_dense_reference(name, Kc):
    """fails on a tree without the mode: jvp_many takes no psd_many there"""
    r = M.point(name)
    L = _lib.lib()
    want_plan = K.host_plan(*K.SHAPES[name][:2])
    assert L.ce_jvp_psd_many_variant(r["eng"]._h) == want_plan["psd_ns_variant"] == L.ce_psd_ns_variant(r["eng"]._h) >= 0
    assert L.ce_jvp_many_variant(r["eng"]._h) == -1 and L.ce_jvp_tri_many_variant(r["eng"]._h) == -1
    M.check_jvp_against_dense(r, Kc)


@pytest.mark.parametrize("Kc", M.KS)
@pytest.mark.parametrize("name", ["psd_mixed", "lqr_like", "row2_n80"])
def test_every_tangent_against_the_loop_of_single_tangent_calls(name, Kc):
    r = M.point(name)
    o, l = M.run_jvp(r, Kc), M.run_jvp(r, Kc, loop=True)
    assert o["kernel"] == "ce_jvp_psd_many" and l["path"] == "loop" and l["kernel"] == "ce_jvp_psd"
    m, lo = o["out"], l["out"]
    assert torch.equal(m[3], lo[3]) and torch.equal(m[4], lo[4]), (name, Kc, m[3], lo[3], m[4], lo[4])
    st = m[3]
    assert ((st & 12) == (st[:1] & 12)).all()          # flags are the matrix's: equal across k
    reg = st == 0
    assert (reg.double().mean(dim=1) >= M.MIN_SHARE).all()
    for i, what in enumerate(("dx", "dy", "ds")):
        e = ((m[i] - lo[i]).abs().amax(dim=2) / (1 + lo[i].abs().amax(dim=2)))[reg]
        print(f"{name} K={Kc}: {what} against the loop {e.max().item():.2e} on status 0; flagged {int((st[0] != 0).sum())} of {st.shape[1]}")
        assert e.max().item() < 1e-6, (name, Kc, what, e.max().item())
        assert torch.equal(m[i][~reg], lo[i][~reg]), (name, Kc, what)          # a flagged pair is the same from-scratch LSQR solve in both routes
    if Kc >= 3:
        un = st[M.ZERO_AT] == 0
        for i in range(3):
            assert (m[i][M.ZERO_AT][un] == 0).all()
            assert torch.equal(m[i][0], m[i][Kc - 1]), (name, Kc, i)          # the repeated tangent, first and last: bit for bit


@pytest.mark.parametrize("which", ("tq", "tA", "both"))
def test_batch_shared_tangents_equal_their_expansion_bit_for_bit(which):
    r = M.point("psd_mixed")
    eng, Kc, B = r["eng"], 3, r["A"].shape[0]
    sA = torch.from_numpy(r["base_tA"][:Kc, 0].copy()).cuda() if which != "tq" else None          # (K, nnz_aug): one row for the batch
    sq = torch.from_numpy(r["base_tq"][:Kc, 0].copy()).cuda() if which != "tA" else None
    shared = eng.jvp_many(r["A_bm"], *r["pt"], sA, sq, q_eval=r["q_t"], psd_many=True, **KW)
    assert eng.last_jvp_kernel == "ce_jvp_psd_many"
    its = eng.last_lsqr_iters
    ex = lambda u: None if u is None else u[:, None, :].expand(Kc, B, u.shape[1]).contiguous()          # noqa: E731
    full = eng.jvp_many(r["A_bm"], *r["pt"], ex(sA), ex(sq), q_eval=r["q_t"], psd_many=True, **KW)
    assert eng.last_jvp_kernel == "ce_jvp_psd_many"
    assert all(torch.equal(u, v) for u, v in zip(shared, full)) and torch.equal(its, eng.last_lsqr_iters)
    assert shared[0].abs().max() > 0


@pytest.mark.parametrize("name", ["psd_mixed", "lqr_like"])
def test_transpose_identity_with_the_many_cotangent_mode(name):
    """<x-bar_k, dx_j> + <y-bar_k, dy_j> == <dA_k, tA_j> + <dq_k, tq_j> for every pair, to 1e-6 (1 + |lhs| + |rhs|), where both modes report status 0"""
    r = M.point(name)
    Kc = 3
    o, v = M.run_jvp(r, Kc), M.run_vjp(r, Kc)
    assert o["kernel"] == "ce_jvp_psd_many" and v["kernel"] == "ce_vjp_psd_many"
    dA, dq, adj = v["out"]
    xb, yb = v["dx"], v["dy"]
    dx, dy, _, st, _ = o["out"]
    lhs = torch.einsum("kbi,jbi->kjb", xb, dx) + torch.einsum("kbi,jbi->kjb", yb, dy)
    rhs = torch.einsum("kbi,jbi->kjb", dA, o["tA"]) + torch.einsum("kbi,jbi->kjb", dq, o["tq"])
    both = (st == 0).all(dim=0) & (adj == 0).all(dim=0)
    assert both.double().mean().item() >= M.MIN_SHARE
    lhs, rhs = lhs[:, :, both].cpu().numpy(), rhs[:, :, both].cpu().numpy()
    e = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
    print(f"{name}: K x K transpose identity {e.max():.2e} on {int(both.sum())} instances")
    assert e.max() < 1e-6 and np.abs(lhs).max() > 1e-3, (name, e.max())


def _flagged_equal_single_calls(eng, A_bm, pt, q_t, tA, tq, many, its, fl):
    """the flagged instances `fl` of a jvp_many result: 12 with iterations > 0 for every k, outputs, status and iteration counts bit for bit those of K single
    ce_jvp_psd calls (every instance's status and iterations equal), and within 1e-6 of ce_jvp_lsqr's answer there"""
    st = many[3]
    assert (st[:, fl] == 12).all() and (st[:, ~fl] == 0).all(), st
    nz = torch.tensor([bool((tA[k] != 0).any() or (tq[k] != 0).any()) for k in range(tA.shape[0])], device=its.device)          # (LSQR takes no iteration on a zero tangent)
    assert (its[nz][:, fl] > 0).all() and (its[~nz] == 0).all() and (its[:, ~fl] == 0).all(), its
    for k in range(tA.shape[0]):
        one = eng.jvp(A_bm, *pt, tA[k], tq[k].t(), q_eval=q_t, psd_ns=True, **KW)
        assert eng.last_jvp_kernel == "ce_jvp_psd"
        assert all(torch.equal(u[k][fl], w[fl]) for u, w in zip(many, one)), k
        assert torch.equal(st[k], one[3]) and torch.equal(its[k], eng.last_lsqr_iters), k
        want = eng.jvp(A_bm, *pt, tA[k], tq[k].t(), q_eval=q_t, path="per_instance", lsqr=TIGHT_LSQR, method="lsqr")
        assert eng.last_jvp_kernel == "ce_jvp_lsqr" and (want[3][fl] == 0).all()
        for i, what in enumerate(("dx", "dy", "ds")):
            e = (many[i][k][fl] - want[i][fl]).abs().max().item() / (1 + want[i][fl].abs().max().item())
            print(f"k={k}: {what} re-solved against the LSQR forward derivative {e:.2e}")
            assert e < 1e-6, (k, what, e)


def test_duplicated_equality_rows_are_flagged_for_every_tangent_and_resolved_in_one_launch():
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
    draws = [_tangents(tpl, int(keep.sum()), seed=seed + 100 + k) for k in range(Kc)]
    tA = torch.stack([d[1] for d in draws]); tq = torch.stack([d[2].t().contiguous() for d in draws])
    A_bm, q_t, pt = torch.from_numpy(A_eval).cuda().t().contiguous(), torch.from_numpy(q_eval).cuda(), tuple(torch.from_numpy(ref[k][keep]).cuda() for k in "xys")
    many = eng.jvp_many(A_bm, *pt, tA, tq, q_eval=q_t, psd_many=True, **KW)
    assert eng.last_jvp_many_path == "many" and eng.last_jvp_kernel == "ce_jvp_psd_many"
    its = eng.last_lsqr_iters
    print("duplicated rows: status", many[3].cpu().numpy().tolist(), "iterations", its.cpu().numpy().tolist())
    _flagged_equal_single_calls(eng, A_bm, pt, q_t, tA, tq, many, its, torch.from_numpy(deg[keep]).cuda())


def test_a_planted_stiff_block_is_flagged_for_every_tangent_and_resolved_in_one_launch():
    """instance 3 of psd_mixed with its first block replaced by U diag(1, 1, -3e-7) U^T (psd_ns_kit.plant_stiff_block): 1 - B = 3e-7 < NS_TRI_STIFF, the threshold
    carried over.  The other instances keep their direct answers bit for bit."""
    r = M.point("psd_mixed")
    eng, inst, Kc = r["eng"], 3, 3
    y, s = K.plant_stiff_block(r["ref"]["y"], r["ref"]["s"], r["cones"], inst)
    assert K.block_states(y[inst] - s[inst], r["cones"])[1] < 1e-5
    pt = (r["pt"][0], torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda())
    base = M.run_jvp(r, Kc)
    many = eng.jvp_many(r["A_bm"], *pt, base["tA"], base["tq"], q_eval=r["q_t"], psd_many=True, **KW)
    assert eng.last_jvp_kernel == "ce_jvp_psd_many"
    its = eng.last_lsqr_iters
    fl = base["out"][3][0] != 0          # (whatever the elimination flags at the unchanged point stays flagged: none on the MI355X)
    assert not fl[inst] and fl.double().mean().item() <= 1 - M.MIN_SHARE
    fl[inst] = True
    _flagged_equal_single_calls(eng, r["A_bm"], pt, r["q_t"], base["tA"], base["tq"], many, its, fl)
    assert all(torch.equal(u[:, ~fl], v[:, ~fl]) for u, v in zip(many, base["out"][:4]))


def test_without_the_flag_the_same_engine_runs_the_loop_bit_for_bit():
    """psd_many=False: K calls of jvp without psd_ns, ce_jvp_lsqr on a PSD template, as before this mode existed"""
    r = M.point("psd_small")
    eng, Kc = r["eng"], 3
    tA, tq = (torch.from_numpy(a).cuda() for a in M.pattern(Kc, r["base_tA"], r["base_tq"]))
    got = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], **KW)
    assert eng.last_jvp_many_path == "loop" and eng.last_jvp_kernel == "ce_jvp_lsqr"
    its = eng.last_lsqr_iters
    for k in range(Kc):
        one = eng.jvp(r["A_bm"], *r["pt"], tA[k], tq[k].t(), q_eval=r["q_t"], **KW)
        assert eng.last_jvp_kernel == "ce_jvp_lsqr"
        assert all(torch.equal(u[k], v) for u, v in zip(got, one)) and torch.equal(its[k], eng.last_lsqr_iters)
    # and with the flag where the one call is not made: method="lsqr" -- the loop, as without it
    kw = dict(KW, method="lsqr")
    a = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], psd_many=True, **kw)
    pa, ia = (eng.last_jvp_many_path, eng.last_jvp_kernel), eng.last_lsqr_iters
    assert pa == ("loop", "ce_jvp_lsqr"), pa
    b = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], **kw)
    assert pa == (eng.last_jvp_many_path, eng.last_jvp_kernel)
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(ia, eng.last_lsqr_iters)


def _same_with_and_without(eng, args, **kw):
    a = eng.jvp_many(*args, psd_many=True, **kw)
    pa = (eng.last_jvp_many_path, eng.last_jvp_kernel)
    ia = eng.last_lsqr_iters
    b = eng.jvp_many(*args, **kw)
    assert pa == (eng.last_jvp_many_path, eng.last_jvp_kernel), pa
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(ia, eng.last_lsqr_iters)
    return pa


def test_the_flag_changes_nothing_on_templates_without_blocks():
    import tri_ns_kit as T
    from test_gpu_parity import gpu_solve
    rng = np.random.default_rng(5)
    Kc = 2
    L = _lib.lib()
    # plain cones: ce_jvp_many's one call, as without the flag (force_loop too: ce_jvp); raw ce_jvp_psd_many on it: CE_E_UNSUPPORTED, the reason named, nothing written
    n, cones, B = 8, {"z": 2, "l": 6, "q": [4]}, 8
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=1)
    eng, A_bm, x, y, s, *_ = gpu_solve(tpl, A, b, c, eps=1e-9, max_iters=200000)
    q_t = torch.from_numpy(tpl.values_from_dense(A, b, c)[1]).cuda()
    tA = torch.from_numpy(rng.standard_normal((Kc, B, tpl.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((Kc, B, n + 1))).cuda()
    assert L.ce_jvp_psd_many_variant(eng._h) == -1
    assert _same_with_and_without(eng, (A_bm, x, y, s, tA, tq), q_eval=q_t, **KW) == ("many", "ce_jvp_many")
    assert _same_with_and_without(eng, (A_bm, x, y, s, tA, tq), q_eval=q_t, force_loop=True, **KW) == ("loop", "ce_jvp")
    f64 = dict(dtype=torch.float64, device="cuda")
    dx = torch.full((Kc, B, n), 7.0, **f64); dy = torch.full((Kc, B, tpl.m), 7.0, **f64); ds = torch.full((Kc, B, tpl.m), 7.0, **f64)
    st = torch.full((Kc, B), -7, dtype=torch.int32, device="cuda"); its = torch.full((Kc, B), -7, dtype=torch.int32, device="cuda")
    A_c = A_bm.contiguous()
    rc = L.ce_jvp_psd_many(eng._h, B, Kc, A_c.data_ptr(), eng.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                           tA.data_ptr(), tA.stride(0), eng.nnz_aug, tq.data_ptr(), tq.stride(0), n + 1, dx.data_ptr(), dy.data_ptr(), ds.data_ptr(), st.data_ptr(),
                           its.data_ptr(), 1e-8, 1e-8, 1e8, 0, None)
    msg = (L.ce_last_error() or b"").decode()
    torch.cuda.synchronize()
    assert rc == -2 and "ce_jvp_psd_many" in msg and "no PSD block" in msg, (rc, msg)
    assert (dx == 7.0).all() and (dy == 7.0).all() and (ds == 7.0).all() and (st == -7).all() and (its == -7).all()
    # a template with triples: the loop of ce_jvp calls, as without the flag
    n, cones, B, seed, _ = T.SHAPES["exp_small"]
    _, _, A, b, c, ref = T.problem("exp_small")
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = _engine(tpl)
    pt = tuple(torch.from_numpy(ref[k]).cuda() for k in "xys")
    tA = torch.from_numpy(rng.standard_normal((Kc, B, tpl.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((Kc, B, n + 1))).cuda()
    assert L.ce_jvp_psd_many_variant(eng._h) == -1
    assert _same_with_and_without(eng, (torch.from_numpy(A_eval).cuda().t().contiguous(), *pt, tA, tq), q_eval=torch.from_numpy(q_eval).cuda(), **KW) == ("loop", "ce_jvp")
    # and the siblings keep refusing a PSD handle, with their messages, before anything is written
    r = M.point("psd_small")
    e, Bp, np_, mp = r["eng"], r["A"].shape[0], r["n"], r["tpl"].m
    tAp = torch.zeros((1, Bp, e.nnz_aug), **f64)
    dxp = torch.full((1, Bp, np_), 7.0, **f64); dyp = torch.full((1, Bp, mp), 7.0, **f64); stp = torch.full((1, Bp), -7, dtype=torch.int32, device="cuda")
    for fn, frag in ((L.ce_jvp_many, "no many-tangent elimination"), (L.ce_jvp_tri_many, "no search-free elimination with triples")):
        rc = fn(e._h, Bp, 1, r["A_bm"].data_ptr(), e.nnz_aug, r["q_t"].data_ptr(), r["q_t"].stride(0), r["q_t"].stride(1), *(t.data_ptr() for t in r["pt"]),
                tAp.data_ptr(), tAp.stride(0), e.nnz_aug, None, 0, 0, dxp.data_ptr(), dyp.data_ptr(), None, stp.data_ptr(), None, 1e-8, 1e-8, 1e8, 0, None)
        assert rc == -2 and frag in (L.ce_last_error() or b"").decode(), (rc, L.ce_last_error())
    rc = L.ce_jvp(e._h, Bp, r["A_bm"].data_ptr(), e.nnz_aug, r["q_t"].data_ptr(), r["q_t"].stride(0), r["q_t"].stride(1), *(t.data_ptr() for t in r["pt"]),
                  tAp.data_ptr(), e.nnz_aug, None, 0, 0, dxp.data_ptr(), dyp.data_ptr(), None, stp.data_ptr(), None, 1e-8, 1e-8, 1e8, 0, None)
    assert rc == -2 and "no search-free elimination" in (L.ce_last_error() or b"").decode(), (rc, L.ce_last_error())
    torch.cuda.synchronize()
    assert (dxp == 7.0).all() and (dyp == 7.0).all() and (stp == -7).all()


def test_the_flag_changes_nothing_on_a_native_quadratic_objective():
    import qp_ns_kit as Q
    from test_quad_objective import _upper_structure
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    n, cones, A, b, c, Pm = Q.instance("small_mixed")
    tpl = P.dense_template(n, cones)
    struct = _upper_structure(n)
    eng = Q.qp_engine(tpl, struct)
    assert eng.qp_native and _lib.lib().ce_jvp_psd_many_variant(eng._h) == -1
    A_bm, q_t, P_bm = Q.device_values(tpl, A, b, c, Pm, struct)
    x, y, s, *_ = eng.solve(A_bm, q_t, make_settings(dict(eps=1e-9, max_iters=200000, acceleration_lookback=0)), P_bm=P_bm)
    B, Kc = A.shape[0], 2
    rng = np.random.default_rng(3)
    tA = torch.from_numpy(rng.standard_normal((Kc, B, tpl.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((Kc, B, n + 1))).cuda()
    assert _same_with_and_without(eng, (A_bm, x, y, s, tA, tq), method="direct", P_bm=P_bm) == ("many", "ce_jvp_qp_many")


def test_empty_batches_and_no_tangent_return_empty_tensors():
    r = M.point("psd_small")
    eng, B, n, m = r["eng"], r["A"].shape[0], r["n"], r["tpl"].m
    z = torch.zeros((0, B, eng.nnz_aug), dtype=torch.float64, device="cuda")
    dx, dy, ds, st = eng.jvp_many(r["A_bm"], *r["pt"], z, None, q_eval=r["q_t"], psd_many=True, **KW)
    assert dx.shape == (0, B, n) and dy.shape == ds.shape == (0, B, m) and st.shape == (0, B) and eng.last_lsqr_iters.shape == (0, B)
    e = torch.zeros((0, m), dtype=torch.float64, device="cuda")
    dx, dy, ds, st = eng.jvp_many(r["A_bm"][:0], e[:, :n], e, e, torch.zeros((2, 0, eng.nnz_aug), dtype=torch.float64, device="cuda"), None, q_eval=r["q_t"][:, :0],
                                  psd_many=True, **KW)
    assert dx.shape == (2, 0, n) and dy.shape == ds.shape == (2, 0, m) and st.shape == (2, 0) and eng.last_lsqr_iters.shape == (2, 0)

"""K tangents at one solution of a template with exponential / power triples on one factorisation per instance: k_backward_ns<..., FWD, ..., TRI, MANY> behind
ce_jvp_tri_many, ConeEngine.jvp_many(tri_many=True) -- and the ONE launch of k_sa_lsqr that re-solves all K right-hand sides of the listed instances (SaWalkMany),
which ce_vjp_many, ce_vjp_tri_many and ce_jvp_many run on as well.

Shapes are tri_ns_kit.SHAPES, all five, at the oracle's points (eps 1e-10, every instance Solved).  K is test_gpu_vjp_many.KS = (1, 3, 17); tangent 1 is all zeros
and tangent 0 is repeated at K - 1 (test_gpu_jvp_many's pattern).  Checked against
  * tri_ns_kit.dense_jvp (a dense numpy solve with the oracle's D) on status-0 instances: 1e-5 worst, 1e-8 median relative to 1 + max |reference| -- the bounds
    test_gpu_tri_jvp.py holds ce_jvp to --, no iteration there, status 0 on >= 80 % for every k;
  * the loop of K ce_jvp calls (force_loop=True): status and iterations equal everywhere, values within 1e-6 on status-0 instances, torch.equal on flagged ones;
  * the zero tangent (exact zeros), the repeat (bit-identical), batch-shared tangents against their expansion (bit-identical);
  * the K x K transpose identity with vjp_many(tri_many=True);
  * duplicated equality rows: 12 for every k, the LSQR forward derivative of the full system under TIGHT_LSQR within test_gpu_tri_jvp.py's bound (1e-6);
  * the one-launch walk on the three modes that had a loop of launches: flagged instances torch.equal to K single vjp / jvp calls;
  * the defaults and refusals that stay."""
import numpy as np
import pytest
import torch

import tri_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_jvp import _engine, _tangents
from test_gpu_vjp_many import KS, K_BEYOND, ZERO_AT, _draw_of, cotangents

pytestmark = pytest.mark.gpu
_CACHE: dict = {}
MIN_SHARE = 0.8
KW = dict(path="per_instance", lsqr=TIGHT_LSQR, method="direct")


def tangents(Kc, base_tA, base_tq):
    """(Kc, B, nnz_aug), (Kc, B, n + 1): draw k at position k, zeros at ZERO_AT and draw 0 again at Kc - 1 when Kc >= 3"""
    tA, tq = base_tA[:Kc].copy(), base_tq[:Kc].copy()
    if Kc >= 3:
        tA[ZERO_AT] = 0.0; tq[ZERO_AT] = 0.0
        tA[Kc - 1] = base_tA[0]; tq[Kc - 1] = base_tq[0]
    return tA, tq


def _point(name):
    """problem, oracle point, engine, K_BEYOND - 1 Gaussian tangent draws (dense and boundary form) and the dense reference of every draw: once per shape, shared"""
    if name in _CACHE:
        return _CACHE[name]
    n, cones, A, b, c, ref = K.problem(name)
    assert (ref["status"] == 1).all(), ref["status"]
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    B = A.shape[0]
    base_tA = np.zeros((K_BEYOND, B, tpl.nnz_aug)); base_tq = np.zeros((K_BEYOND, B, n + 1)); want = []
    for k in range(K_BEYOND - 1):
        (dA, db, dc), tA_bm, tq = _tangents(tpl, B, seed=K.SHAPES[name][3] + 100 + k)
        base_tA[k] = tA_bm.cpu().numpy(); base_tq[k] = tq.cpu().numpy().T
        w = K.dense_jvp(A, ref["x"], ref["y"], ref["s"], dA, db, dc, cones)
        assert w[3].all(), (name, k, w[4])          # zero left out
        want.append(w[:3])
    r = dict(name=name, n=n, cones=cones, tpl=tpl, A=A, b=b, c=c, ref=ref, eng=_engine(tpl), A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(),
             q_t=torch.from_numpy(q_eval).cuda(), pt=tuple(torch.from_numpy(ref[k]).cuda() for k in "xys"), base_tA=base_tA, base_tq=base_tq, want=want, runs={})
    _CACHE[name] = r
    return r


def _run(r, Kc, loop=False):
    """jvp_many(tri_many=True) -- or the loop of ce_jvp calls -- for Kc tangents at the shape's point (once each): tensors (dx, dy, ds, status, iters) on the device"""
    key = (Kc, loop)
    if key in r["runs"]:
        return r["runs"][key]
    eng = r["eng"]
    tA, tq = tangents(Kc, r["base_tA"], r["base_tq"])
    tAt, tqt = torch.from_numpy(tA).cuda(), torch.from_numpy(tq).cuda()
    got = eng.jvp_many(r["A_bm"], *r["pt"], tAt, tqt, q_eval=r["q_t"], tri_many=not loop, force_loop=loop, **KW)
    out = dict(path=eng.last_jvp_many_path, kernel=eng.last_jvp_kernel, out=tuple(got) + (eng.last_lsqr_iters,), tA=tAt, tq=tqt)
    torch.cuda.synchronize()
    r["runs"][key] = out
    return out


def _rel(got, want):
    return np.abs(got - want).max(axis=-1) / (1 + np.abs(want).max(axis=-1))


@pytest.mark.parametrize("Kc", KS)
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_every_tangent_against_the_dense_reference(name, Kc):
    """fails on a tree without the mode: jvp_many takes no tri_many there"""
    r = _point(name)
    o = _run(r, Kc)
    L = _lib.lib()
    assert o["path"] == "many" and o["kernel"] == "ce_jvp_tri_many", (o["path"], o["kernel"])
    assert L.ce_jvp_tri_many_variant(r["eng"]._h) == K.SHAPES[name][4] == L.ce_tri_ns_variant(r["eng"]._h)
    assert L.ce_jvp_many_variant(r["eng"]._h) == -1
    dx, dy, ds, st, its = (t.cpu().numpy() for t in o["out"])
    n, m, B = r["n"], r["tpl"].m, r["A"].shape[0]
    assert dx.shape == (Kc, B, n) and dy.shape == ds.shape == (Kc, B, m) and st.shape == its.shape == (Kc, B)
    for k in range(Kc):
        d = _draw_of(Kc, k)
        reg = st[k] == 0
        assert reg.mean() >= MIN_SHARE, (name, Kc, k, reg.mean(), np.bincount(st[k]))
        assert (its[k][reg] == 0).all(), (name, Kc, k)
        if d is None:
            continue
        for got, want, what in zip((dx[k], dy[k], ds[k]), r["want"][d], ("dx", "dy", "ds")):
            e = _rel(got, want)[reg]
            print(f"{name} K={Kc} k={k}: {what} worst {e.max():.2e} median {np.median(e):.2e}, compared {reg.mean():.3f}, status counts {np.bincount(st[k]).tolist()}")
            assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, Kc, k, what, e.max(), np.median(e))


@pytest.mark.parametrize("Kc", KS)
@pytest.mark.parametrize("name", ["exp_pow_mixed", "E"])
def test_every_tangent_against_the_loop_of_single_tangent_calls(name, Kc):
    r = _point(name)
    o, l = _run(r, Kc), _run(r, Kc, loop=True)
    assert o["kernel"] == "ce_jvp_tri_many" and l["path"] == "loop" and l["kernel"] == "ce_jvp"
    m, lo = o["out"], l["out"]
    assert torch.equal(m[3], lo[3]) and torch.equal(m[4], lo[4]), (name, Kc, m[3], lo[3], m[4], lo[4])
    st = m[3]
    assert ((st & (4 | 8)) == (st[:1] & (4 | 8))).all()          # flags are the matrix's: equal across k
    reg = st == 0
    assert (reg.double().mean(dim=1) >= MIN_SHARE).all()
    for i, what in enumerate(("dx", "dy", "ds")):
        e = ((m[i] - lo[i]).abs().amax(dim=2) / (1 + lo[i].abs().amax(dim=2)))[reg]
        print(f"{name} K={Kc}: {what} against the loop {e.max().item():.2e} on status 0; flagged {int((st[0] != 0).sum())} of {st.shape[1]}")
        assert e.max().item() < 1e-6, (name, Kc, what, e.max().item())
        assert torch.equal(m[i][~reg], lo[i][~reg]), (name, Kc, what)          # a flagged pair is the same from-scratch LSQR solve in both routes
    if Kc >= 3:
        un = st[ZERO_AT] == 0
        for i in range(3):
            assert (m[i][ZERO_AT][un] == 0).all()
            assert torch.equal(m[i][0], m[i][Kc - 1]), (name, Kc, i)          # the repeated tangent, first and last: bit for bit


@pytest.mark.parametrize("which", ("tq", "tA", "both"))
def test_batch_shared_tangents_equal_their_expansion_bit_for_bit(which):
    r = _point("exp_pow_mixed")
    eng, Kc, B = r["eng"], 3, r["A"].shape[0]
    sA = torch.from_numpy(r["base_tA"][:Kc, 0].copy()).cuda() if which != "tq" else None          # (K, nnz_aug): one row for the batch
    sq = torch.from_numpy(r["base_tq"][:Kc, 0].copy()).cuda() if which != "tA" else None
    shared = eng.jvp_many(r["A_bm"], *r["pt"], sA, sq, q_eval=r["q_t"], tri_many=True, **KW)
    assert eng.last_jvp_kernel == "ce_jvp_tri_many"
    its = eng.last_lsqr_iters
    ex = lambda u: None if u is None else u[:, None, :].expand(Kc, B, u.shape[1]).contiguous()
    full = eng.jvp_many(r["A_bm"], *r["pt"], ex(sA), ex(sq), q_eval=r["q_t"], tri_many=True, **KW)
    assert eng.last_jvp_kernel == "ce_jvp_tri_many"
    assert all(torch.equal(u, v) for u, v in zip(shared, full)) and torch.equal(its, eng.last_lsqr_iters)
    assert shared[0].abs().max() > 0


@pytest.mark.parametrize("name", ["exp_pow_mixed", "E"])
def test_transpose_identity_with_the_many_cotangent_mode(name):
    """<x-bar_k, dx_j> + <y-bar_k, dy_j> == <dA_k, tA_j> + <dq_k, tq_j> for every pair, to 1e-6 (1 + |lhs| + |rhs|), where both modes report status 0"""
    r = _point(name)
    eng, Kc = r["eng"], 3
    o = _run(r, Kc)
    rng = np.random.default_rng(K.SHAPES[name][3] + 1)
    xb, yb = (torch.from_numpy(a).cuda() for a in cotangents(Kc, rng.standard_normal((K_BEYOND,) + r["ref"]["x"].shape), rng.standard_normal((K_BEYOND,) + r["ref"]["y"].shape)))
    dA, dq, adj = eng.vjp_many(r["A_bm"], *r["pt"], xb, yb, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], tri_many=True)
    assert eng.last_vjp_kernel == "ce_vjp_tri_many"
    dx, dy, _, st, _ = o["out"]
    lhs = torch.einsum("kbi,jbi->kjb", xb, dx) + torch.einsum("kbi,jbi->kjb", yb, dy)
    rhs = torch.einsum("kbi,jbi->kjb", dA, o["tA"]) + torch.einsum("kbi,jbi->kjb", dq, o["tq"])
    both = (st == 0).all(dim=0) & (adj == 0).all(dim=0)
    assert both.double().mean().item() >= MIN_SHARE
    lhs, rhs = lhs[:, :, both].cpu().numpy(), rhs[:, :, both].cpu().numpy()
    e = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
    print(f"{name}: K x K transpose identity {e.max():.2e} on {int(both.sum())} instances")
    assert e.max() < 1e-6 and np.abs(lhs).max() > 1e-3, (name, e.max())


def test_duplicated_equality_rows_are_flagged_for_every_tangent_and_resolved():
    """the construction of test_gpu_tri_jvp.py::test_duplicated_equality_rows_are_flagged_and_resolved with K = 3: status 12 for every k on the degenerate instances,
    0 on the others; the degenerate ones within that test's 1e-6 of that test's reference, the LSQR forward derivative of the full system under TIGHT_LSQR
    (ce_jvp_lsqr, which must itself report status 0 there: the oracle has no forward derivative of its own, its LSQR is what that kernel is pinned on)"""
    from oracle import oracle
    n, cones, B, seed, _ = K.SHAPES["exp_pow_mixed"]
    Kc = 3
    A, b, c = P.generate(n, cones, B, seed=seed)
    deg = np.arange(B) % 2 == 0
    A[deg, 1, :] = A[deg, 0, :]; b[deg, 1] = b[deg, 0]
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)
    keep = ref["status"] == 1
    assert keep.mean() >= 0.8, keep.mean()
    A, b, c, deg = A[keep], b[keep], c[keep], deg[keep]
    ref = {k: v[keep] for k, v in ref.items()}
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = _engine(tpl)
    draws = [_tangents(tpl, A.shape[0], seed=seed + 100 + k) for k in range(Kc)]
    tA = torch.stack([d[1] for d in draws]); tq = torch.stack([d[2].t().contiguous() for d in draws])
    A_bm, q_t, pt = torch.from_numpy(A_eval).cuda().t().contiguous(), torch.from_numpy(q_eval).cuda(), tuple(torch.from_numpy(ref[k]).cuda() for k in "xys")
    dx, dy, ds, st = eng.jvp_many(A_bm, *pt, tA, tq, q_eval=q_t, tri_many=True, **KW)
    assert eng.last_jvp_many_path == "many" and eng.last_jvp_kernel == "ce_jvp_tri_many"
    its = eng.last_lsqr_iters.cpu().numpy()
    st = st.cpu().numpy()
    for k in range(Kc):
        print(f"duplicated rows k={k}: status {st[k].tolist()} iterations {its[k].tolist()}")
        assert (st[k][deg] == 12).all() and (st[k][~deg] == 0).all(), (k, st[k])
        assert (its[k][deg] > 0).all() and (its[k][~deg] == 0).all(), (k, its[k])
        want = eng.jvp(A_bm, *pt, tA[k], tq[k].t(), path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t, method="lsqr")
        assert eng.last_jvp_kernel == "ce_jvp_lsqr" and (want[3].cpu().numpy()[deg] == 0).all()
        for got, w, what in zip((dx, dy, ds), want, ("dx", "dy", "ds")):
            w = w.cpu().numpy()[deg]
            e = np.abs(got[k].cpu().numpy()[deg] - w).max() / (1 + np.abs(w).max())
            print(f"duplicated rows k={k}: {what} re-solved against the LSQR forward derivative {e:.2e}")
            assert e < 1e-6, (k, what, e)


def _flagged_equal_single_jvp(eng, A_bm, pt, q_t, tA, tq, many, its, kernel, need_flagged):
    """the flagged instances of a jvp_many result against K single jvp calls: outputs, status and iteration counts, bit for bit.  need_flagged: the construction
    flags by design (duplicated rows); the LP vertices of this seed happen to be regular for the elimination on the MI355X (none flagged, as test_gpu_jvp_many.py
    prints), so that case pins the status alone"""
    assert eng.last_jvp_kernel == kernel
    fl = (many[3][0] & 8) != 0
    assert (fl.any() or not need_flagged) and not fl.all()
    for k in range(tA.shape[0]):
        one = eng.jvp(A_bm, *pt, tA[k], tq[k].t(), q_eval=q_t, **KW)
        assert eng.last_jvp_kernel == "ce_jvp"
        assert all(torch.equal(u[k][fl], v[fl]) for u, v in zip(many, one)) and torch.equal(its[k][fl], eng.last_lsqr_iters[fl]), k
        assert torch.equal(many[3][k], one[3]) and torch.equal(its[k], eng.last_lsqr_iters), k          # status and iterations: every instance
        assert (eng.last_lsqr_iters[fl] > 0).all()
    return int(fl.sum())


@pytest.mark.parametrize("construction", ("lp_vertex", "duplicated_rows"))
def test_one_launch_walk_ce_jvp_many(construction):
    from test_gpu_jvp_direct import _point as direct_point

    def mutate(A, b):
        deg = np.arange(A.shape[0]) % 2 == 0
        A[deg, 2, :] = A[deg, 0, :]; b[deg, 2] = b[deg, 0]
        return deg
    n, cones, B, seed, mut = {"lp_vertex": (10, {"z": 0, "l": 30, "q": []}, 64, 9, None), "duplicated_rows": (12, {"z": 4, "l": 8, "q": [5]}, 24, 11, mutate)}[construction]
    r = direct_point(n, cones, B, seed, eps=1e-10, min_solved=0.8, mutate=mut)
    eng, Bk, Kc = r["eng"], int(r["keep"].sum()), 3
    rng = np.random.default_rng(seed + 7)
    tA = torch.from_numpy(rng.standard_normal((Kc, Bk, r["tpl"].nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((Kc, Bk, n + 1))).cuda()
    many = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], **KW)
    assert eng.last_jvp_many_path == "many"
    nfl = _flagged_equal_single_jvp(eng, r["A_bm"], r["pt"], r["q_t"], tA, tq, many, eng.last_lsqr_iters, "ce_jvp_many", construction == "duplicated_rows")
    print(f"ce_jvp_many, {construction}: {nfl} of {Bk} flagged instances equal K single ce_jvp calls bit for bit")


@pytest.mark.parametrize("construction", ("lp_vertex", "duplicated_rows"))
def test_one_launch_walk_ce_vjp_many(construction):
    from oracle import oracle
    from test_gpu_parity import gpu_solve
    n, cones, B, seed = {"lp_vertex": (10, {"z": 0, "l": 30, "q": []}, 64, 9), "duplicated_rows": (12, {"z": 4, "l": 8, "q": [5]}, 24, 11)}[construction]
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=seed)
    if construction == "duplicated_rows":
        deg = np.arange(B) % 2 == 0
        A[deg, 2, :] = A[deg, 0, :]; b[deg, 2] = b[deg, 0]
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)
    keep = ref["status"] == 1
    assert keep.mean() > 0.8
    A, b, c = A[keep], b[keep], c[keep]
    eng, A_bm, *_ = gpu_solve(tpl, A, b, c, eps=1e-10, max_iters=200000)
    pt = tuple(torch.from_numpy(ref[k][keep]).cuda() for k in "xys")
    q_t = torch.from_numpy(tpl.values_from_dense(A, b, c)[1]).cuda()
    rng = np.random.default_rng(seed + 1)
    Kc = 3
    dx = torch.from_numpy(rng.standard_normal((Kc,) + tuple(pt[0].shape))).cuda(); dy = torch.from_numpy(rng.standard_normal((Kc,) + tuple(pt[1].shape))).cuda()
    dA, dq, adj = eng.vjp_many(A_bm, *pt, dx, dy, path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t)
    assert eng.last_vjp_many_path == "many" and eng.last_vjp_kernel == "ce_vjp_many"
    fl = (adj[0] & 8) != 0
    assert (fl.any() or construction == "lp_vertex") and not fl.all()          # (the LP vertices of this seed: none flagged on the MI355X; the status is still pinned)
    for k in range(Kc):
        a1, q1, s1 = eng.vjp(A_bm, *pt, dx[k], dy[k], path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t)
        assert torch.equal(dA[k][fl], a1.t()[fl]) and torch.equal(dq[k][fl], q1.t()[fl]) and torch.equal(adj[k], s1), k
    print(f"ce_vjp_many, {construction}: {int(fl.sum())} of {int(keep.sum())} flagged instances equal K single ce_vjp calls bit for bit")


def test_one_launch_walk_ce_vjp_tri_many():
    """duplicated equality rows (test_gpu_vjp_tri_many.py's construction): the pivoting kernel behind ce_vjp flags them too and hands them to the same LSQR kernel, so
    the re-solved answers of the two routes are the same solves"""
    from oracle import oracle
    n, cones, B, seed, _ = K.SHAPES["exp_pow_mixed"]
    Kc = 3
    A, b, c = P.generate(n, cones, B, seed=seed)
    deg = np.arange(B) % 2 == 0
    A[deg, 1, :] = A[deg, 0, :]; b[deg, 1] = b[deg, 0]
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)
    keep = ref["status"] == 1
    assert keep.mean() >= 0.8, keep.mean()
    A, b, c, deg = A[keep], b[keep], c[keep], torch.from_numpy(deg[keep]).cuda()
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = _engine(tpl)
    A_bm = torch.from_numpy(A_eval).cuda().t().contiguous(); q_t = torch.from_numpy(q_eval).cuda()
    pt = tuple(torch.from_numpy(ref[k][keep]).cuda() for k in "xys")
    rng = np.random.default_rng(seed + 12)
    dx = torch.from_numpy(rng.standard_normal((Kc,) + tuple(pt[0].shape))).cuda(); dy = torch.from_numpy(rng.standard_normal((Kc,) + tuple(pt[1].shape))).cuda()
    dA, dq, adj = eng.vjp_many(A_bm, *pt, dx, dy, path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t, tri_many=True)
    assert eng.last_vjp_kernel == "ce_vjp_tri_many"
    assert (adj[:, deg] == 12).all()
    for k in range(Kc):
        a1, q1, s1 = eng.vjp(A_bm, *pt, dx[k], dy[k], path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t)
        assert (s1[deg] == 12).all(), s1
        assert torch.equal(dA[k][deg], a1.t()[deg]) and torch.equal(dq[k][deg], q1.t()[deg]) and torch.equal(adj[k][deg], s1[deg]), k


def test_without_the_flag_the_same_engine_runs_the_loop_bit_for_bit():
    r = _point("exp_pow_mixed")
    eng, Kc = r["eng"], 3
    tA, tq = (torch.from_numpy(a).cuda() for a in tangents(Kc, r["base_tA"], r["base_tq"]))
    got = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], **KW)
    assert eng.last_jvp_many_path == "loop" and eng.last_jvp_kernel == "ce_jvp"
    its = eng.last_lsqr_iters
    for k in range(Kc):
        one = eng.jvp(r["A_bm"], *r["pt"], tA[k], tq[k].t(), q_eval=r["q_t"], **KW)
        assert all(torch.equal(u[k], v) for u, v in zip(got, one)) and torch.equal(its[k], eng.last_lsqr_iters)
    # and with the flag where the one call is not made: force_loop, method="lsqr"
    for kw in (dict(KW, force_loop=True), dict(KW, method="lsqr")):
        a = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], tri_many=True, **kw)
        pa = (eng.last_jvp_many_path, eng.last_jvp_kernel)
        assert pa == ("loop", "ce_jvp_lsqr" if kw["method"] == "lsqr" else "ce_jvp"), (kw, pa)
        ia = eng.last_lsqr_iters
        b = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], **kw)
        assert pa == (eng.last_jvp_many_path, eng.last_jvp_kernel)
        assert all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(ia, eng.last_lsqr_iters), kw


def _same_with_and_without(eng, args, **kw):
    a = eng.jvp_many(*args, tri_many=True, **kw)
    pa = (eng.last_jvp_many_path, eng.last_jvp_kernel)
    ia = eng.last_lsqr_iters
    b = eng.jvp_many(*args, **kw)
    assert pa == (eng.last_jvp_many_path, eng.last_jvp_kernel), pa
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b)) and torch.equal(ia, eng.last_lsqr_iters)
    return pa


def test_the_flag_changes_nothing_on_templates_without_triples():
    from test_gpu_parity import gpu_solve
    rng = np.random.default_rng(5)
    Kc = 2
    # plain cones: ce_jvp_many's one call, as without the flag
    n, cones, B = 8, {"z": 2, "l": 6, "q": [4]}, 8
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=1)
    eng, A_bm, x, y, s, *_ = gpu_solve(tpl, A, b, c, eps=1e-9, max_iters=200000)
    q_t = torch.from_numpy(tpl.values_from_dense(A, b, c)[1]).cuda()
    tA = torch.from_numpy(rng.standard_normal((Kc, B, tpl.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((Kc, B, n + 1))).cuda()
    assert _lib.lib().ce_jvp_tri_many_variant(eng._h) == -1
    assert _same_with_and_without(eng, (A_bm, x, y, s, tA, tq), q_eval=q_t, **KW) == ("many", "ce_jvp_many")
    # raw ce_jvp_tri_many on it: CE_E_UNSUPPORTED, the entry point and the reason named, nothing written
    f64 = dict(dtype=torch.float64, device="cuda")
    dx = torch.full((Kc, B, n), 7.0, **f64); dy = torch.full((Kc, B, tpl.m), 7.0, **f64); ds = torch.full((Kc, B, tpl.m), 7.0, **f64)
    st = torch.full((Kc, B), -7, dtype=torch.int32, device="cuda"); its = torch.full((Kc, B), -7, dtype=torch.int32, device="cuda")
    A_c = A_bm.contiguous()
    rc = _lib.lib().ce_jvp_tri_many(eng._h, B, Kc, A_c.data_ptr(), eng.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                                    tA.data_ptr(), tA.stride(0), eng.nnz_aug, tq.data_ptr(), tq.stride(0), n + 1, dx.data_ptr(), dy.data_ptr(), ds.data_ptr(), st.data_ptr(),
                                    its.data_ptr(), 1e-8, 1e-8, 1e8, 0, None)
    msg = (_lib.lib().ce_last_error() or b"").decode()
    torch.cuda.synchronize()
    assert rc == -2 and "ce_jvp_tri_many" in msg and "no exponential / power cone" in msg, (rc, msg)
    assert (dx == 7.0).all() and (dy == 7.0).all() and (ds == 7.0).all() and (st == -7).all() and (its == -7).all()
    # a PSD template: the loop
    n, cones, B = 4, {"z": 1, "s": [3]}, 4
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=2)
    eng, A_bm, x, y, s, *_ = gpu_solve(tpl, A, b, c, eps=1e-9, max_iters=200000)
    q_t = torch.from_numpy(tpl.values_from_dense(A, b, c)[1]).cuda()
    tA = torch.from_numpy(rng.standard_normal((Kc, B, tpl.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((Kc, B, n + 1))).cuda()
    assert _lib.lib().ce_jvp_tri_many_variant(eng._h) == -1
    assert _same_with_and_without(eng, (A_bm, x, y, s, tA, tq), q_eval=q_t, path="per_instance", lsqr=TIGHT_LSQR, method="lsqr") == ("loop", "ce_jvp_lsqr")


def test_the_flag_changes_nothing_on_a_native_quadratic_objective():
    import qp_ns_kit as Q
    from test_quad_objective import _upper_structure
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    n, cones, A, b, c, Pm = Q.instance("small_mixed")
    tpl = P.dense_template(n, cones)
    struct = _upper_structure(n)
    eng = Q.qp_engine(tpl, struct)
    assert eng.qp_native and _lib.lib().ce_jvp_tri_many_variant(eng._h) == -1
    A_bm, q_t, P_bm = Q.device_values(tpl, A, b, c, Pm, struct)
    x, y, s, *_ = eng.solve(A_bm, q_t, make_settings(dict(eps=1e-9, max_iters=200000, acceleration_lookback=0)), P_bm=P_bm)
    B, Kc = A.shape[0], 2
    rng = np.random.default_rng(3)
    tA = torch.from_numpy(rng.standard_normal((Kc, B, tpl.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((Kc, B, n + 1))).cuda()
    assert _same_with_and_without(eng, (A_bm, x, y, s, tA, tq), method="direct", P_bm=P_bm) == ("many", "ce_jvp_qp_many")          # (what test_gpu_jvp_qp_many.py sees there)


def test_empty_batches_and_no_tangent_return_empty_tensors():
    r = _point("exp_small")
    eng, B, n, m = r["eng"], r["A"].shape[0], r["n"], r["tpl"].m
    z = torch.zeros((0, B, eng.nnz_aug), dtype=torch.float64, device="cuda")
    dx, dy, ds, st = eng.jvp_many(r["A_bm"], *r["pt"], z, None, q_eval=r["q_t"], tri_many=True, **KW)
    assert dx.shape == (0, B, n) and dy.shape == ds.shape == (0, B, m) and st.shape == (0, B) and eng.last_lsqr_iters.shape == (0, B)
    e = torch.zeros((0, m), dtype=torch.float64, device="cuda")
    dx, dy, ds, st = eng.jvp_many(r["A_bm"][:0], e[:, :n], e, e, torch.zeros((2, 0, eng.nnz_aug), dtype=torch.float64, device="cuda"), None, q_eval=r["q_t"][:, :0],
                                  tri_many=True, **KW)
    assert dx.shape == (2, 0, n) and dy.shape == ds.shape == (2, 0, m) and st.shape == (2, 0) and eng.last_lsqr_iters.shape == (2, 0)

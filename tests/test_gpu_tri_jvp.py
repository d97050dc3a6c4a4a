"""The forward-mode derivative by direct elimination on templates with exponential / power triples: k_backward_ns<..., FWD, TRI> behind ce_jvp
(ce_tri_ns_variant >= 0), ConeEngine.jvp(method="direct").  A triple's D Pi is diagonalised, its three rows are rotated into that basis and become equalities,
dropped rows or one weighted row of the reduced Hessian; the LSQR re-solve behind the kernel serves the flagged instances.  Checked against
  * a dense numpy solve of [[0, A^T D], [A, D - I]] with D from the oracle's dproj_exp / dproj_pow (tri_ns_kit.dense_jvp): no instance is left out, every
    system has condition <= 1e11 (<= 8.9e2 in fact);
  * the LSQR forward derivative (ce_jvp_lsqr) under the tight rule, to the bounds of test_gpu_jvp_direct._check_regular_against_lsqr;
  * the transpose identity against the pivoting adjoint (k_backward_rt), central differences of the GPU solve, duplicated equality rows, null tangents;
  * the refusals that stay (PSD template, quadratic objective inside the kernels).
All linearisation points are the oracle's solutions at eps 1e-10; every instance of every shape is Solved."""
import ctypes as C

import numpy as np
import pytest
import torch

import tri_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_jvp import _engine, _tangents
from test_gpu_jvp_direct import _both, _check_regular_against_lsqr

pytestmark = pytest.mark.gpu
_CACHE: dict = {}


def _point(name):
    """engine, batch-major values, q_eval, the oracle's (x, y, s) on the device, the tangents (dense and boundary form) and both forward derivatives: once per shape"""
    if name not in _CACHE:
        n, cones, A, b, c, ref = K.problem(name)
        assert (ref["status"] == 1).all(), ref["status"]
        tpl = P.dense_template(n, cones)
        A_eval, q_eval = tpl.values_from_dense(A, b, c)
        dense_t, tA_bm, tq = _tangents(tpl, A.shape[0], seed=K.SHAPES[name][3] + 100)
        r = dict(tpl=tpl, eng=_engine(tpl), A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(), q_t=torch.from_numpy(q_eval).cuda(),
                 pt=tuple(torch.from_numpy(ref[k]).cuda() for k in ("x", "y", "s")), tA_bm=tA_bm, tq=tq, dense_t=dense_t, A=A, ref=ref, cones=cones)
        r["direct"], r["lsqr"] = _both(r)          # (asserts that ce_jvp and ce_jvp_lsqr ran)
        _CACHE[name] = r
    return _CACHE[name]


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_direct_equals_the_dense_reference_and_lsqr(shape):
    """fails on a build without the triples in the elimination: ce_jvp refuses the handle there and _both sees ce_jvp_lsqr run in its place"""
    r = _point(shape)
    L = _lib.lib()
    assert L.ce_tri_ns_variant(r["eng"]._h) == K.SHAPES[shape][4] and L.ce_adjoint_ns_variant(r["eng"]._h) < 0
    assert r["eng"].plan()["tri_ns_variant"] == K.SHAPES[shape][4] and r["eng"].plan()["ns_variant"] == -1
    d, l = r["direct"], r["lsqr"]
    reg, _ = _check_regular_against_lsqr(d, l, 0.8)          # status 0 with 0 iterations on >= 80 %, and equal to LSQR there
    dA, db, dc = r["dense_t"]
    ref = r["ref"]
    want = K.dense_jvp(r["A"], ref["x"], ref["y"], ref["s"], dA, db, dc, r["cones"])
    print("condition of the dense systems: max", want[4].max())
    assert want[3].all(), want[4]          # zero left out
    states = np.concatenate([K.triple_states(ref["y"][i] - ref["s"][i], r["cones"]) for i in range(reg.size)])
    snapped = (states < 1e-9) | (states > 1 - 1e-9)
    counts = (int((states.min(axis=1) > 1 - 1e-9).sum()), int((states.max(axis=1) < 1e-9).sum()), int((~snapped[:, 1]).sum()),
              int((snapped.all(axis=1) & (states[:, 0] < 1e-9) & (states[:, 2] > 1 - 1e-9)).sum()))
    print("triples: D = I, D = 0, boundary with a middle eigenvalue, boundary snapped flat:", counts)
    assert min(counts) > 0, counts          # every shape keeps all four states (equality, dropped and weighted rows, and the snapped branches) in front of the kernel
    for k, name in enumerate(("dx", "dy", "ds")):
        e = (np.abs(d[k] - want[k]).max(axis=1) / (1 + np.abs(want[k]).max(axis=1)))[reg]
        print(f"{name} vs dense: max {e.max():.3e} median {np.median(e):.3e}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, e.max(), np.median(e))


@pytest.mark.parametrize("shape", ["exp_pow_mixed", "E"])
def test_transpose_identity_against_the_pivoting_adjoint(shape):
    """<x-bar, dx> + <y-bar, dy>  ==  <dA_eval, tA_eval> + <dq_eval, tq_eval>  per instance, to 1e-6 (1 + |lhs| + |rhs|), where both eliminations solved directly"""
    r = _point(shape)
    eng, (x, y, s) = r["eng"], r["pt"]
    rng = np.random.default_rng(K.SHAPES[shape][3] + 2)
    xb = torch.from_numpy(rng.standard_normal(tuple(x.shape))).cuda(); yb = torch.from_numpy(rng.standard_normal(tuple(y.shape))).cuda()
    dx, dy, ds, st = eng.jvp(r["A_bm"], x, y, s, r["tA_bm"], r["tq"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    assert eng.last_jvp_kernel == "ce_jvp"
    dA, dq, adj = eng.vjp(r["A_bm"], x, y, s, xb, yb, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"])
    torch.cuda.synchronize()
    st, adj = st.cpu().numpy(), adj.cpu().numpy()
    both = (st == 0) & (adj == 0)
    print("jvp status counts", np.bincount(st), "adjoint status counts", np.bincount(adj), "compared", both.mean())
    assert both.mean() >= 0.8
    lhs = ((xb * dx).sum(dim=1) + (yb * dy).sum(dim=1)).cpu().numpy()[both]
    rhs = ((dA.t() * r["tA_bm"]).sum(dim=1) + (dq * r["tq"]).sum(dim=0)).cpu().numpy()[both]
    print("transpose identity: max |lhs - rhs| / (1 + |lhs| + |rhs|) =", (np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))).max())
    assert (np.abs(lhs - rhs) < 1e-6 * (1 + np.abs(lhs) + np.abs(rhs))).all(), (lhs, rhs)
    assert np.abs(lhs).max() > 1e-3


def test_direct_jvp_is_the_derivative_of_the_gpu_solution_map():
    """recipe and bound of test_gpu_jvp_direct.py::test_direct_jvp_is_the_derivative_of_the_gpu_solution_map (central differences of eng.solve at eps 1e-11,
    h = 1e-5).  Seed 14: of the seeds 0 .. 19 of P.generate at this shape it keeps every instance farthest from a kind change at the oracle's point -- no
    eigenvalue of a triple's D that is not snapped to 0 / 1 lies within 7.1e-2 of either (the rule asks for 1e-3), the nonnegative rows keep |v_i| >= 0.13 and the
    second-order cone | |z| -+ t | >= 6.7e-2: a difference quotient across a kind change would be wrong, not the kernel."""
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    n, cones, B = 12, {"z": 2, "l": 6, "q": [4], "ep": 2, "p": [0.3]}, 8
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=14)
    eng = _engine(tpl)
    assert _lib.lib().ce_tri_ns_variant(eng._h) == 0
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
    """exp_pow_mixed with its second equality row a copy of the first on every second instance: the row elimination drops it, flags the instance (4) and the LSQR
    launch behind the kernel re-solves it (8) -- bounds of test_gpu_jvp_direct.py::test_duplicated_equality_rows_are_flagged_and_resolved"""
    from oracle import oracle
    n, cones, B, seed, _ = K.SHAPES["exp_pow_mixed"]
    A, b, c = P.generate(n, cones, B, seed=seed)
    deg = np.arange(B) % 2 == 0
    A[deg, 1, :] = A[deg, 0, :]; b[deg, 1] = b[deg, 0]
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)
    keep = ref["status"] == 1
    assert keep.mean() >= 0.8, keep.mean()
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A[keep], b[keep], c[keep])
    _, tA_bm, tq = _tangents(tpl, int(keep.sum()), seed=seed + 100)
    r = dict(eng=_engine(tpl), A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(), q_t=torch.from_numpy(q_eval).cuda(),
             pt=tuple(torch.from_numpy(ref[k][keep]).cuda() for k in ("x", "y", "s")), tA_bm=tA_bm, tq=tq)
    deg = deg[keep]
    d, l = _both(r)
    print("status", d[3], "iters", d[4])
    assert (d[3][deg] == 12).all() and (d[4][deg] > 0).all(), (d[3], d[4])
    assert (l[3][deg] == 0).all()
    for k, name in enumerate(("dx", "dy", "ds")):
        e = np.abs(d[k][deg] - l[k][deg]).max() / (1 + np.abs(l[k][deg]).max())
        print(name, "re-solved vs lsqr:", e)
        assert e < 1e-6, (name, e)
    ok = ~deg & (l[3] == 0) & (d[3] == 0)
    assert ok.sum() >= 0.8 * (~deg).sum()
    e = np.max([np.abs(d[k] - l[k]).max(axis=1) / (1 + np.abs(l[k]).max(axis=1)) for k in range(3)], axis=0)[ok]
    assert e.max() < 1e-5 and np.median(e) < 1e-8, (e.max(), np.median(e))


def test_null_tangents_give_exact_zeros():
    r = _point("exp_pow_mixed")
    eng = r["eng"]
    dx, dy, ds, st = eng.jvp(r["A_bm"], *r["pt"], None, None, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    assert eng.last_jvp_kernel == "ce_jvp"
    reg = torch.from_numpy(r["direct"][3] == 0).cuda()
    assert reg.float().mean() >= 0.8
    assert (dx[reg] == 0).all() and (dy[reg] == 0).all() and (ds[reg] == 0).all() and (st[reg] == 0).all() and (eng.last_lsqr_iters[reg] == 0).all()
    assert torch.isfinite(dx).all() and torch.isfinite(dy).all() and torch.isfinite(ds).all()


def _raw_ce_jvp(eng, B=3):
    zf = torch.zeros((B, max(eng.n, eng.m, eng.nnz_aug) + 1), dtype=torch.float64, device="cuda"); zi = torch.zeros((B,), dtype=torch.int32, device="cuda")
    p, ip = zf.data_ptr(), zi.data_ptr()
    rc = _lib.lib().ce_jvp(eng._h, B, p, eng.nnz_aug, None, 0, 0, p, p, p, p, eng.nnz_aug, None, 0, 0, p, p, p, ip, ip, 1e-8, 1e-8, 1e8, 0,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, _lib.lib().ce_last_error().decode()


def test_refusals_that_stay():
    """a PSD template and a handle with the quadratic objective inside the kernels are refused by ce_jvp as before, message for message"""
    import qp_ns_kit as Q
    eng = _engine(P.dense_template(4, {"z": 1, "s": [3]}))
    assert _lib.lib().ce_tri_ns_variant(eng._h) < 0 and _lib.lib().ce_adjoint_ns_variant(eng._h) < 0
    rc, msg = _raw_ce_jvp(eng)
    assert rc == -2 and msg == "ce_jvp: this template has no search-free elimination (PSD / exponential / power cones, or n > 108); use ce_jvp_lsqr", msg
    # a PSD block beside triples: no elimination either
    eng = _engine(P.dense_template(6, {"z": 1, "l": 2, "s": [2], "ep": 1}))
    assert _lib.lib().ce_tri_ns_variant(eng._h) < 0
    assert _raw_ce_jvp(eng)[0] == -2
    n = 6
    qeng = Q.qp_engine(P.dense_template(n, {"z": 2, "l": 4, "q": []}), Q.full_structure(n))
    assert qeng.qp_native and _lib.lib().ce_tri_ns_variant(qeng._h) < 0
    rc, msg = _raw_ce_jvp(qeng)
    assert rc == -2 and msg == "forward derivative: not available with a quadratic objective inside the kernels; use the epigraph form (cone form) of the problem", msg
    # plain-cone templates keep their own variant and have none of this one
    eng = _engine(P.dense_template(8, {"z": 4, "l": 6, "q": [4]}))
    assert _lib.lib().ce_adjoint_ns_variant(eng._h) == 0 and _lib.lib().ce_tri_ns_variant(eng._h) < 0

"""The forward-mode derivative by direct elimination on templates with PSD blocks: k_backward_ns<..., FWD, ..., PSD> behind ce_jvp_psd (ce_psd_ns_variant >= 0),
ConeEngine.jvp(method="direct", psd_ns=True).  Per block smat(v_c) = U Lambda U^T by the workgroup's Jacobi sweeps; the block's rows of A are rotated into the
eigenbasis of D Pi and become equalities, dropped rows or one weighted row each of the reduced Hessian; the LSQR re-solve behind the kernel serves the flagged
instances.  Checked against
  * a dense numpy solve of [[0, A^T D], [A, D - I]] with D from numpy.linalg.eigh and the B_ab rule (psd_ns_kit.dense_jvp): no instance is left out;
  * the LSQR forward derivative (ce_jvp_lsqr) under the tight rule, to the bounds of test_gpu_jvp_direct._check_regular_against_lsqr;
  * the transpose identity against the pivoting adjoint (k_backward_rt<PSD>), a duplicated equality row, a planted stiff block, null tangents, a block of order 1;
  * today's route without the flag.
All linearisation points are the oracle's solutions at eps 1e-10; every instance of every shape is Solved."""
import numpy as np
import pytest
import torch

import psd_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_jvp import _engine, _tangents
from test_gpu_jvp_direct import _check_regular_against_lsqr

pytestmark = pytest.mark.gpu
_CACHE: dict = {}


def _both(r, tA_bm="given", tq="given", pt=None):
    """(dx, dy, ds, status, iters) as numpy arrays of ce_jvp_psd and of ce_jvp_lsqr under the tight rule, on the same tangents (test_gpu_jvp_direct._both with the flag)"""
    eng = r["eng"]
    tA_bm = r["tA_bm"] if isinstance(tA_bm, str) else tA_bm
    tq = r["tq"] if isinstance(tq, str) else tq
    out = {}
    for method, kernel in (("direct", "ce_jvp_psd"), ("lsqr", "ce_jvp_lsqr")):
        got = eng.jvp(r["A_bm"], *(pt or r["pt"]), tA_bm, tq, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method=method, psd_ns=True)
        assert eng.last_jvp_kernel == kernel, (method, eng.last_jvp_kernel)
        torch.cuda.synchronize()
        out[method] = tuple(t.cpu().numpy() for t in got) + (eng.last_lsqr_iters.cpu().numpy(),)
    return out["direct"], out["lsqr"]


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
        r["direct"], r["lsqr"] = _both(r)          # (asserts that ce_jvp_psd and ce_jvp_lsqr ran)
        _CACHE[name] = r
    return _CACHE[name]


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_direct_equals_the_dense_reference_and_lsqr(shape):
    """fails on a build without the PSD mode: ce_jvp_psd does not exist there"""
    r = _point(shape)
    L = _lib.lib()
    eng = r["eng"]
    want_plan = K.host_plan(*K.SHAPES[shape][:2])
    assert L.ce_psd_ns_variant(eng._h) == want_plan["psd_ns_variant"] >= 0 and L.ce_psd_ns_lds(eng._h) == want_plan["psd_ns_lds"] > 0
    assert eng.psd_ns_plan() == {"psd_ns_variant": want_plan["psd_ns_variant"], "psd_ns_lds": want_plan["psd_ns_lds"]}
    assert eng.plan()["ns_variant"] == -1 and eng.plan()["tri_ns_variant"] == -1 and L.ce_adjoint_ns_variant(eng._h) < 0 and L.ce_tri_ns_variant(eng._h) < 0
    d, l = r["direct"], r["lsqr"]
    reg, _ = _check_regular_against_lsqr(d, l, 0.8)          # status 0 with 0 iterations on >= 80 %, and equal to LSQR there
    dA, db, dc = r["dense_t"]
    ref = r["ref"]
    want = K.dense_jvp(r["A"], ref["x"], ref["y"], ref["s"], dA, db, dc, r["cones"])
    print("condition of the dense systems: max", want[4].max())
    assert want[3].all(), want[4]          # zero left out
    counts, margin, kw = K.state_counts(shape)
    print("blocks: D = I, D = 0, mixed:", counts, "smallest min(B, 1 - B):", margin, "largest weighted-row count:", kw)
    assert margin > 1e-5          # the stiff rule flags nothing here: the 0.8 share is a condition, not a measurement
    if shape in ("psd_mixed", "psd_only"):
        assert min(counts) > 0, counts          # all three states (equality, dropped and weighted rows) in front of the kernel
    for k, name in enumerate(("dx", "dy", "ds")):
        e = (np.abs(d[k] - want[k]).max(axis=1) / (1 + np.abs(want[k]).max(axis=1)))[reg]
        print(f"{name} vs dense: max {e.max():.3e} median {np.median(e):.3e}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, e.max(), np.median(e))


@pytest.mark.parametrize("shape", ["psd_mixed", "lqr_like"])
def test_transpose_identity_against_the_pivoting_adjoint(shape):
    """<x-bar, dx> + <y-bar, dy>  ==  <dA_eval, tA_eval> + <dq_eval, tq_eval>  per instance, to 1e-6 (1 + |lhs| + |rhs|), where both eliminations solved directly"""
    r = _point(shape)
    eng, (x, y, s) = r["eng"], r["pt"]
    rng = np.random.default_rng(K.SHAPES[shape][3] + 2)
    xb = torch.from_numpy(rng.standard_normal(tuple(x.shape))).cuda(); yb = torch.from_numpy(rng.standard_normal(tuple(y.shape))).cuda()
    dx, dy, ds, st = eng.jvp(r["A_bm"], x, y, s, r["tA_bm"], r["tq"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct", psd_ns=True)
    assert eng.last_jvp_kernel == "ce_jvp_psd"
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


def test_duplicated_equality_rows_are_flagged_and_resolved():
    """psd_mixed with its second equality row a copy of the first on every second instance: the row elimination drops it, flags the instance (4) and the LSQR launch
    behind the kernel re-solves it (8) -- bounds of test_gpu_tri_jvp.py::test_duplicated_equality_rows_are_flagged_and_resolved"""
    from oracle import oracle
    n, cones, B, seed = K.SHAPES["psd_mixed"]
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


def test_a_planted_stiff_block_is_flagged_and_resolved():
    """instance 3 of psd_mixed with its first block replaced by U diag(1, 1, -3e-7) U^T: two weighted rows with 1 - B = 3e-7 < NS_TRI_STIFF.  The forward derivative
    flags the instance and the re-solve serves it: status 4 | 8, iterations > 0, the answer ce_jvp_lsqr's own (the same kernel under the same rule).  The point is
    not optimal and need not be: the derivative system is linear algebra at the point given.  The other instances keep their direct answers."""
    r = _point("psd_mixed")
    ref, inst = r["ref"], 3
    y, s = K.plant_stiff_block(ref["y"], ref["s"], r["cones"], inst)
    _, margin = K.block_states(y[inst] - s[inst], r["cones"])
    assert margin < 1e-5, margin
    pt = (r["pt"][0], torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda())
    d, l = _both(r, pt=pt)
    print("status", d[3], "iters", d[4])
    assert d[3][inst] == 12 and d[4][inst] > 0, (d[3][inst], d[4][inst])
    for k, name in enumerate(("dx", "dy", "ds")):
        e = np.abs(d[k][inst] - l[k][inst]).max() / (1 + np.abs(l[k][inst]).max())
        print(name, "re-solved vs lsqr:", e)
        assert e < 1e-6, (name, e)
    others = np.arange(d[3].size) != inst
    assert (d[3][others] == r["direct"][3][others]).all()
    for k in range(3):
        assert np.array_equal(d[k][others], r["direct"][k][others])


def test_null_tangents_give_exact_zeros():
    r = _point("psd_mixed")
    eng = r["eng"]
    dx, dy, ds, st = eng.jvp(r["A_bm"], *r["pt"], None, None, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct", psd_ns=True)
    assert eng.last_jvp_kernel == "ce_jvp_psd"
    reg = torch.from_numpy(r["direct"][3] == 0).cuda()
    assert reg.float().mean() >= 0.8
    assert (dx[reg] == 0).all() and (dy[reg] == 0).all() and (ds[reg] == 0).all() and (st[reg] == 0).all() and (eng.last_lsqr_iters[reg] == 0).all()
    assert torch.isfinite(dx).all() and torch.isfinite(dy).all() and torch.isfinite(ds).all()


def test_a_block_of_order_one_is_a_nonnegative_row():
    """{z 2, l 5, s [1]} against {z 2, l 6}: the same rows, the last one a PSD block of order 1 -- its one eigenvalue decides as a nonnegative row does (B = 1 for
    v > 0, else 0), the rotation is the identity.  ce_jvp_psd on the first equals ce_jvp on the second to 1e-12 (1 + |.|): the same elimination in another row order
    of the same arithmetic."""
    from oracle import oracle
    n, B = 6, 16
    plain, psd = {"z": 2, "l": 6, "q": []}, {"z": 2, "l": 5, "q": [], "s": [1]}
    A, b, c = P.generate(n, plain, B, seed=2)
    ref = oracle.solve_batch(A, b, c, plain, eps=1e-10, max_iters=200000)
    assert (ref["status"] == 1).all()
    v_last = ref["y"][:, -1] - ref["s"][:, -1]
    assert (v_last > 0).any() and (v_last <= 0).any(), v_last          # both decisions
    got = {}
    for name, cones in (("plain", plain), ("psd", psd)):
        tpl = P.dense_template(n, cones)
        A_eval, q_eval = tpl.values_from_dense(A, b, c)
        _, tA_bm, tq = _tangents(tpl, B, seed=7)
        eng = _engine(tpl)
        out = eng.jvp(torch.from_numpy(A_eval).cuda().t().contiguous(), *(torch.from_numpy(ref[k]).cuda() for k in ("x", "y", "s")), tA_bm, tq,
                      path="per_instance", lsqr=TIGHT_LSQR, q_eval=torch.from_numpy(q_eval).cuda(), method="direct", psd_ns=(name == "psd"))
        assert eng.last_jvp_kernel == ("ce_jvp_psd" if name == "psd" else "ce_jvp")
        torch.cuda.synchronize()
        got[name] = tuple(t.cpu().numpy() for t in out)
    both = (got["plain"][3] == 0) & (got["psd"][3] == 0)
    assert (got["plain"][3] == got["psd"][3]).all() and both.mean() >= 0.8, (got["plain"][3], got["psd"][3])
    for k, name in enumerate(("dx", "dy", "ds")):
        e = np.abs(got["psd"][k][both] - got["plain"][k][both]).max() / (1 + np.abs(got["plain"][k][both]).max())
        print(name, "order-1 block vs nonnegative row:", e)
        assert e < 1e-12, (name, e)


def test_without_the_flag_the_lsqr_call_runs_as_today():
    r = _point("psd_small")
    eng = r["eng"]
    got = eng.jvp(r["A_bm"], *r["pt"], r["tA_bm"], r["tq"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    assert eng.last_jvp_kernel == "ce_jvp_lsqr"
    torch.cuda.synchronize()
    for k in range(3):
        assert np.array_equal(got[k].cpu().numpy(), r["lsqr"][k])

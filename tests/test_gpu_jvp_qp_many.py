"""K tangents at one solution on one factorisation per instance, QP kind: k_backward_ns<..., FWD, QP, ..., MANY> behind ce_jvp_qp_many, ConeEngine.jvp_many(P_bm=, tP=).

The cases of test_gpu_qp_jvp.py (its _case is shared: one oracle solve per case in a session) and the l = 2n family of plan_kit at both sides of its two row edges,
n = 28 / 29 and n = 60 / 61, at planted points (ns_edge_kit).  K = 1, 3, 17 with tangents of A, q and P; tangent 0 is repeated at position K - 1 (bit-identical) and
tangent 1 is all zeros (exact zeros on unflagged instances).  Checked against
  * the loop of K ce_jvp_qp calls (force_loop=True): 1e-6 relative to 1 + max |reference| on every instance, equal status, no iterations;
  * qp_ns_kit's dense solve on the draws 0, 2 and 15, at test_gpu_qp_jvp.py's bounds (max < 1e-5, median < 1e-8 on at least 80 % of a batch);
  * a flagged instance (a duplicated equality row): status 4 for every k, never 4 | 8, no iterations, finite numbers."""
import numpy as np
import pytest
import torch

import ns_edge_kit as E
import plan_kit as pk
import qp_ns_kit as Q
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from test_gpu_jvp_many import _rel
from test_gpu_qp_jvp import CASES, _case
from test_gpu_vjp_many import K_BEYOND, KS, ZERO_AT, _draw_of
from test_quad_objective import _p_values, _upper_structure

pytestmark = pytest.mark.gpu

L2N = {f"l2n_n{n}": n for n in (28, 29, 60, 61)}
L2N_ROW = {28: 0, 29: 1, 60: 1, 61: 2}
ALL = list(CASES) + list(L2N)
DENSE_DRAWS = (0, 2, K_BEYOND - 2)
_T: dict = {}


def _planted(name):
    n = L2N[name]
    shape = ("qp", n, {"z": 0, "l": 2 * n, "q": []}, ())
    pt = E.point("jvp_qp_many:" + name, shape, B=8)
    tpl = P.dense_template(n, shape[2])
    ps = pk.ns_pstruct("qp", n)
    struct = (ps[0], ps[1], (n, n))
    eng = Q.qp_engine(tpl, struct)
    A_bm, q_t, P_bm = Q.device_values(tpl, pt["A"], pt["b"], pt["c"], pt["Pm"], struct)
    return dict(name=name, tpl=tpl, cones=shape[2], A=pt["A"], Pm=pt["Pm"], struct=struct, ref=dict(x=pt["x"], y=pt["y"], s=pt["s"], status=np.ones(8, int)), eng=eng,
                A_bm=A_bm, P_bm=P_bm, pt=tuple(torch.from_numpy(pt[k]).cuda() for k in "xys"))


def _shape(name):
    """the case's shared point, K_BEYOND dense Gaussian tangent draws (tA on the template's pattern, tP symmetric) in the boundary's coordinates, and the dense
    answers of DENSE_DRAWS: computed once per case, shared, not changed"""
    if name in _T:
        return _T[name]
    r = _planted(name) if name in L2N else _case(name)
    tpl, A = r["tpl"], r["A"]
    B, m, n = A.shape
    rng = np.random.default_rng(500 + len(name) + n)
    pat = np.zeros((m, n), bool); cols = np.repeat(np.arange(n + 1), np.diff(tpl.indptr)); on = cols < n
    pat[np.asarray(tpl.indices)[on], cols[on]] = True
    base_tA, base_tq, base_tP, dense = [], [], [], {}
    for d in range(K_BEYOND):
        tA, tb, tc, tP = rng.standard_normal(A.shape) * pat[None], rng.standard_normal((B, m)), rng.standard_normal((B, n)), Q.sym_tangent(B, n, 900 + d)
        tA_eval, tq_eval = tpl.values_from_dense(tA, tb, tc)
        base_tA.append(tA_eval.T); base_tq.append(tq_eval.T); base_tP.append(Q.p_tangent_values(tP, r["struct"]))
        if d in DENSE_DRAWS:
            dense[d] = Q.dense_jvp(A, r["Pm"], r["ref"]["x"], r["ref"]["y"], r["ref"]["s"], tA, tb, tc, tP, r["cones"])
    t = dict(r=r, B=B, base=tuple(np.ascontiguousarray(np.stack(a)) for a in (base_tA, base_tq, base_tP)), dense=dense, runs={})
    _T[name] = t
    return t


def tangents(K, base):
    out = [a[:K].copy() for a in base]
    if K >= 3:
        for a, b in zip(out, base):
            a[ZERO_AT] = 0.0; a[K - 1] = b[0]
    return out


def _run(t, K):
    if K in t["runs"]:
        return t["runs"][K]
    r = t["r"]; eng = r["eng"]
    tA, tq, tP = (torch.from_numpy(a).cuda() for a in tangents(K, t["base"]))
    many = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, method="direct", P_bm=r["P_bm"], tP=tP)
    path, kernel, its = eng.last_jvp_many_path, eng.last_jvp_kernel, eng.last_lsqr_iters
    loop = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, method="direct", P_bm=r["P_bm"], tP=tP, force_loop=True)
    assert eng.last_jvp_many_path == "loop" and eng.last_jvp_kernel == "ce_jvp_qp"
    its_l = eng.last_lsqr_iters
    torch.cuda.synchronize()
    out = dict(path=path, kernel=kernel, many=tuple(u.cpu().numpy() for u in many + (its,)), loop=tuple(u.cpu().numpy() for u in loop + (its_l,)))
    t["runs"][K] = out
    return out


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ALL)
def test_every_tangent_against_the_loop_and_the_dense_solve(name, K):
    t = _shape(name)
    o = _run(t, K)
    r = t["r"]
    Lb = _lib.lib()
    assert o["path"] == "many" and o["kernel"] == "ce_jvp_qp_many"
    row = Lb.ce_jvp_qp_many_variant(r["eng"]._h)
    assert row == Lb.ce_qp_ns_variant(r["eng"]._h) >= 0 and Lb.ce_jvp_many_variant(r["eng"]._h) == -1
    if name in L2N:
        assert row == L2N_ROW[L2N[name]], (name, row)
    m, l = o["many"], o["loop"]
    assert (m[3] == l[3]).all() and (m[4] == 0).all() and (l[4] == 0).all() and ((m[3] & ~4) == 0).all(), (name, K, m[3], l[3])
    assert (m[3] == m[3][:1]).all()          # flagged is the matrix's
    for i, what in enumerate(("dx", "dy", "ds")):
        assert np.isfinite(m[i]).all()
        e = _rel(m[i], l[i])
        print(f"{name} K={K} row {row}: {what} against the loop {e.max():.2e}, flagged {int((m[3][0] != 0).sum())}")
        assert e.max() < 1e-6, (name, K, what, e.max())
    if K >= 3:
        un = m[3][ZERO_AT] == 0
        for i in range(3):
            assert (m[i][ZERO_AT][un] == 0).all()
            assert np.array_equal(m[i][0], m[i][K - 1]), (name, K, i)
    for k in range(K):
        d = _draw_of(K, k)
        if d not in t["dense"]:
            continue
        want = t["dense"][d]
        sel = (m[3][k] == 0) & want[3] & (r["ref"]["status"] == 1)
        assert sel.mean() >= 0.8, (name, K, k, sel.mean())
        e = np.max([_rel(m[i][k], want[i]) for i in range(3)], axis=0)[sel]
        print(f"{name} K={K} k={k}: against the dense solve max {e.max():.3e} median {np.median(e):.3e}, compared {sel.mean():.3f}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, K, k, e.max(), np.median(e))


@pytest.mark.parametrize("which", ("tP", "tq", "all"))
def test_null_and_batch_shared_tangents(which):
    t = _shape("small_mixed")
    r = t["r"]; eng = r["eng"]
    K, B = 3, t["B"]
    sA, sq, sP = (torch.from_numpy(a[:K, 0].copy()).cuda() for a in t["base"])          # one row for the batch
    if which == "tP":
        sA = sq = None
    elif which == "tq":
        sA = sP = None
    kw = dict(method="direct", P_bm=r["P_bm"])
    shared = eng.jvp_many(r["A_bm"], *r["pt"], sA, sq, tP=sP, **kw)
    assert eng.last_jvp_many_path == "many"
    ex = lambda u: None if u is None else u[:, None, :].expand(K, B, u.shape[1]).contiguous()
    full = eng.jvp_many(r["A_bm"], *r["pt"], ex(sA), ex(sq), tP=ex(sP), **kw)
    assert all(torch.equal(u, v) for u, v in zip(shared, full)) and shared[0].abs().max() > 0
    loop = eng.jvp_many(r["A_bm"], *r["pt"], sA, sq, tP=sP, force_loop=True, **kw)
    for u, v in zip(shared[:3], loop[:3]):
        e = ((u - v).abs().amax(dim=2) / (1 + v.abs().amax(dim=2))).max().item()
        assert e < 1e-6, (which, e)
    assert torch.equal(shared[3], loop[3])


def test_a_flagged_instance_keeps_status_four_for_every_tangent():
    """test_gpu_qp_jvp.py's duplicated equality row on the small mixed shape: every second instance"""
    from oracle import oracle
    n, cones, A, b, c, Pm = Q.instance("small_mixed")
    deg = np.arange(A.shape[0]) % 2 == 0
    A[deg, 1, :] = A[deg, 0, :]; b[deg, 1] = b[deg, 0]
    tpl = P.dense_template(n, cones); struct = _upper_structure(n)
    ref = oracle.solve_batch(A, b, c, cones, P=Pm, eps=1e-10, max_iters=200000)
    assert (ref["status"] == 1).mean() >= 0.9
    eng = Q.qp_engine(tpl, struct)
    A_bm, q_t, P_bm = Q.device_values(tpl, A, b, c, Pm, struct)
    t = _shape("small_mixed")
    K = 3
    tA, tq, tP = (torch.from_numpy(a).cuda() for a in tangents(K, t["base"]))
    pt = tuple(torch.from_numpy(ref[k]).cuda() for k in "xys")
    out = eng.jvp_many(A_bm, *pt, tA, tq, method="direct", P_bm=P_bm, tP=tP)
    assert eng.last_jvp_many_path == "many"
    its = eng.last_lsqr_iters
    loop = eng.jvp_many(A_bm, *pt, tA, tq, method="direct", P_bm=P_bm, tP=tP, force_loop=True)
    torch.cuda.synchronize()
    st = out[3].cpu().numpy()
    for k in range(K):
        assert (st[k][deg] == 4).all() and (st[k][~deg] == 0).all(), (k, st[k])
    assert (its == 0).all() and torch.equal(out[3], loop[3])
    for u, v in zip(out[:3], loop[:3]):
        assert torch.isfinite(u).all()
        e = ((u - v).abs().amax(dim=2) / (1 + v.abs().amax(dim=2)))[:, torch.from_numpy(~deg).cuda()].max().item()
        assert e < 1e-6, e


def test_the_plain_entry_point_refuses_a_native_qp_template():
    t = _shape("small_mixed")
    r = t["r"]; eng = r["eng"]
    K, B = 2, t["B"]
    f64 = dict(dtype=torch.float64, device="cuda")
    z = torch.zeros((K, B, max(eng.n, eng.m, eng.nnz_aug)), **f64); st = torch.zeros((K, B), dtype=torch.int32, device="cuda")
    rc = _lib.lib().ce_jvp_many(eng._h, B, K, r["A_bm"].data_ptr(), eng.nnz_aug, None, 0, 0, *(u.data_ptr() for u in r["pt"]), z.data_ptr(), z.stride(0), z.stride(1),
                                None, 0, 0, z.data_ptr(), z.data_ptr(), None, st.data_ptr(), None, 1e-8, 1e-8, 1e8, 0, None)
    assert rc == -2 and b"ce_jvp_qp_many" in _lib.lib().ce_last_error()

"""K cotangents at one solution on one factorisation per instance, quadratic objective inside the kernels: k_backward_ns<..., QP, ..., MANY> without FWD behind
ce_vjp_qp_many, ConeEngine.vjp_many(P_bm=, qp_many=True).

The cases of test_gpu_qp_jvp.py (its _case is shared: one oracle solve per case in a session; ragged_cones on the full structure, the others on one triangle -- the
dP doubling differs) and the l = 2n family of plan_kit at both sides of its two row edges, n = 28 / 29 and n = 60 / 61, at planted points (ns_edge_kit, the points
of test_gpu_jvp_qp_many.py).  K = 1, 3, 17 Gaussian cotangents; cotangent 0 is repeated at position K - 1 (bit-identical) and cotangent 1 is all zeros (exact zeros
in dA, dq and dP on unflagged instances).  Checked against
  * the loop of K ce_vjp_qp calls (qp_many=False), the pivoting kernel -- another algorithm: dA, dq, dP within 1e-6 relative to 1 + max |reference| on the
    instances unflagged by both (test_gpu_ns_adjoint.py's bound for search-free against pivoting);
  * the oracle's dense adjoint with P on the draws 0, 2 and 15: max < 1e-5, median < 1e-8 on the instances with oracle status 1, cond(qp_ns_kit.kkt_matrix) <= 1e11
    and no flag -- at least 80 % of every batch;
  * the forward twin ce_jvp_qp_many:  <dx_k, jvp.dx_j> + <dy_k, jvp.dy_j> = <dA_k, tA_j> + <dq_k, tq_j> + <dP_k, tP_j>  in the boundary's coordinates.  No block
    changes sign: include/cone_engine.h gives ce_vjp_qp's outputs and ce_jvp_qp's tangents in the same boundary convention (dA_eval = [-dA.data, db[b_idx]],
    dq_eval = [dc, 0], dP in the structure's order with a one-triangle entry standing for both matrix entries on both sides), the identity
    test_gpu_qp_jvp.py::test_transpose_identity_... already holds ce_vjp_qp to.  Bound: 1e-6 relative to 1 + the larger side, on unflagged instances;
  * dy = None against an explicit zero dy (bit for bit), a flagged instance (status 4 for every k, never 4 | 8, finite), the refusals."""
import numpy as np
import pytest
import torch

import ns_edge_kit as E
import qp_ns_kit as Q
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from test_gpu_jvp_qp_many import ALL, L2N, L2N_ROW
from test_gpu_jvp_qp_many import _shape as _tangent_shape
from test_gpu_jvp_qp_many import tangents
from test_gpu_qp_jvp import _case
from test_gpu_vjp_many import K_BEYOND, KS, ZERO_AT, _draw_of, cotangents
from test_quad_objective import _p_values, _upper_structure

pytestmark = pytest.mark.gpu

ORACLE_DRAWS = (0, 2, K_BEYOND - 2)
_T: dict = {}


def _rel(got, want):
    """per (k,) instance: max |got - want| / (1 + max |want|) over the last axis"""
    return np.abs(got - want).max(axis=-1) / (1 + np.abs(want).max(axis=-1))


def _one_triangle(struct):
    idx, ptr, _ = struct
    cols = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return bool((idx <= cols).all() or (idx >= cols).all())


def _dp_values(dP, struct):
    """the oracle's dense symmetric dP (B, n, n) in the structure's order: a one-triangle entry off the diagonal stands for both matrix entries and takes both shares"""
    idx, ptr, _ = struct
    cols = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    vals = _p_values(dP, struct)
    return vals * np.where(idx != cols, 2.0, 1.0) if _one_triangle(struct) else vals


def _shape(name):
    """the case's shared point, K_BEYOND Gaussian cotangent draws, the oracle's dense adjoint of ORACLE_DRAWS in the boundary's coordinates and the oracle-only
    part of the comparison mask (status 1, cond of the KKT matrix <= 1e11): computed once per case, shared, not changed"""
    if name in _T:
        return _T[name]
    from oracle import oracle
    r = dict(_tangent_shape(name)["r"])          # (the forward twin's case: one engine, one oracle solve per case in a session)
    if name in L2N:
        n2 = L2N[name]
        pt = E.point("jvp_qp_many:" + name, ("qp", n2, {"z": 0, "l": 2 * n2, "q": []}, ()), B=8)          # (the point test_gpu_jvp_qp_many.py planted: its b and c)
        assert pt["A"] is r["A"]
        r["b"], r["c"] = pt["b"], pt["c"]
    tpl, A, ref = r["tpl"], r["A"], r["ref"]
    B, m, n = A.shape
    rng = np.random.default_rng(700 + len(name) + n)
    base_dx = rng.standard_normal((K_BEYOND, B, n)); base_dy = rng.standard_normal((K_BEYOND, B, m))
    cols = np.repeat(np.arange(n + 1), np.diff(tpl.indptr))
    want = {}
    for d in ORACLE_DRAWS:
        g = oracle.adjoint_batch(A, r["b"], r["c"], r["cones"], ref["x"], ref["y"], ref["s"], base_dx[d], base_dy[d], P=r["Pm"], mode="dense")
        dA = np.stack([-g["dA"][:, i, j] if j < n else g["db"][:, i] for i, j in zip(tpl.indices, cols)], axis=1)
        want[d] = (dA, g["dc"], _dp_values(g["dP"], r["struct"]))
    cond_ok = np.zeros(B, bool)
    for i in range(B):
        J, _ = Q.kkt_matrix(A[i], r["Pm"][i], ref["y"][i] - ref["s"][i], r["cones"])
        cond_ok[i] = bool(np.isfinite(J).all()) and np.linalg.cond(J) <= 1e11
    t = dict(r=r, B=B, n=n, m=m, base_dx=base_dx, base_dy=base_dy, want=want, oracle_ok=cond_ok & (ref["status"] == 1), runs={})
    _T[name] = t
    return t


def _run(t, K):
    if K in t["runs"]:
        return t["runs"][K]
    r = t["r"]; eng = r["eng"]
    dx, dy = (torch.from_numpy(a).cuda() for a in cotangents(K, t["base_dx"], t["base_dy"]))
    many = eng.vjp_many(r["A_bm"], *r["pt"], dx, dy, path="per_instance", P_bm=r["P_bm"], qp_many=True)
    path, kernel = eng.last_vjp_many_path, eng.last_vjp_kernel
    loop = eng.vjp_many(r["A_bm"], *r["pt"], dx, dy, path="per_instance", P_bm=r["P_bm"])
    assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None
    torch.cuda.synchronize()
    out = dict(path=path, kernel=kernel, many=tuple(u.cpu().numpy() for u in many), loop=tuple(u.cpu().numpy() for u in loop))
    t["runs"][K] = out
    return out


def test_both_structures_of_P_appear():
    tri = {name: _one_triangle(_case(name)["struct"]) for name in ("ragged_cones", "small_mixed")}
    assert tri == {"ragged_cones": False, "small_mixed": True}, tri


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ALL)
def test_every_cotangent_against_the_loop_and_the_oracle(name, K):
    t = _shape(name)
    o = _run(t, K)
    r = t["r"]; eng = r["eng"]
    Lb = _lib.lib()
    assert o["path"] == "many" and o["kernel"] == "ce_vjp_qp_many"
    row = Lb.ce_vjp_qp_many_variant(eng._h)
    assert row == Lb.ce_qp_ns_variant(eng._h) >= 0 and Lb.ce_vjp_many_variant(eng._h) == -1
    if name in L2N:
        assert row == L2N_ROW[L2N[name]], (name, row)
    m, l = o["many"], o["loop"]
    B, n = t["B"], t["n"]
    assert m[0].shape == (K, B, eng.nnz_aug) and m[1].shape == (K, B, n + 1) and m[2].shape == (K, B) and m[3].shape == (K, B, eng.nnz_p)
    st = m[2]
    assert ((st & ~4) == 0).all() and (st == st[:1]).all(), (name, K, st)          # no bits beyond 4; flagged is the matrix's
    assert (m[1][:, :, n] == 0).all()
    both = (st == 0) & (l[2] == 0)
    for i, what in ((0, "dA"), (1, "dq"), (3, "dP")):
        assert np.isfinite(m[i]).all()
        e = _rel(m[i], l[i])
        print(f"{name} K={K} row {row}: {what} against the loop {e[both].max() if both.any() else 0.0:.2e}, flagged {int((st[0] != 0).sum())} / loop {int((l[2][0] != 0).sum())}")
        assert (e[both] < 1e-6).all(), (name, K, what, e[both].max())
    if K >= 3:
        un = st[ZERO_AT] == 0
        for i in (0, 1, 3):
            assert (m[i][ZERO_AT][un] == 0).all(), (name, K, i)
            assert np.array_equal(m[i][0], m[i][K - 1]), (name, K, i)
    if name == "inactive_box":
        assert (st == 0).all(), st
    for k in range(K):
        d = _draw_of(K, k)
        if d not in t["want"]:
            continue
        sel = t["oracle_ok"] & (st[k] == 0)
        print(f"{name} K={K} k={k}: oracle-only mask {t['oracle_ok'].mean():.3f}, compared {sel.mean():.3f}")
        assert t["oracle_ok"].mean() >= 0.8 and sel.mean() >= 0.8, (name, K, k, t["oracle_ok"].mean(), sel.mean())
        want = t["want"][d]
        e = np.max([_rel(m[0][k], want[0]), _rel(m[1][k][:, :n], want[1]), _rel(m[3][k], want[2])], axis=0)[sel]
        print(f"{name} K={K} k={k}: against the oracle max {e.max():.3e} median {np.median(e):.3e}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, K, k, e.max(), np.median(e))


@pytest.mark.parametrize("name", ALL)
def test_duality_with_the_forward_twin(name):
    """every pair (cotangent k, tangent j), K = J = 3 (the zero cotangent and the zero tangent among them); see the module docstring for the signs"""
    t = _shape(name)
    tt = _tangent_shape(name)
    r = t["r"]; eng = r["eng"]
    K = 3
    o = _run(t, K)
    dx, dy = cotangents(K, t["base_dx"], t["base_dy"])
    tA, tq, tP = tangents(K, tt["base"])
    jv = eng.jvp_many(r["A_bm"], *r["pt"], *(torch.from_numpy(a).cuda() for a in (tA, tq)), method="direct", P_bm=r["P_bm"], tP=torch.from_numpy(tP).cuda())
    assert eng.last_jvp_many_path == "many" and eng.last_jvp_kernel == "ce_jvp_qp_many"
    torch.cuda.synchronize()
    jdx, jdy, _, jst = (u.cpu().numpy() for u in jv)
    dA, dq, st, dP = o["many"]
    lhs = np.einsum("kbi,jbi->kjb", dx, jdx) + np.einsum("kbi,jbi->kjb", dy, jdy)
    rhs = np.einsum("kbi,jbi->kjb", dA, tA) + np.einsum("kbi,jbi->kjb", dq, tq) + np.einsum("kbi,jbi->kjb", dP, tP)
    un = (st[0] == 0) & (jst[0] == 0)
    assert un.any(), name
    e = np.abs(lhs - rhs) / (1 + np.maximum(np.abs(lhs), np.abs(rhs)))
    print(f"{name}: max |lhs - rhs| / (1 + larger side) = {e[:, :, un].max():.3e}, max |lhs| = {np.abs(lhs[:, :, un]).max():.3e}")
    assert (e[:, :, un] < 1e-6).all(), (name, e[:, :, un].max())
    assert np.abs(lhs[:, :, un]).max() > 1e-3
    # the P block alone carries weight: a wrong doubling could not hide behind the others
    assert np.abs(np.einsum("kbi,jbi->kjb", dP, tP)[:, :, un]).max() > 1e-3


def test_a_null_dy_is_the_zero_cotangent():
    t = _shape("small_mixed")
    r = t["r"]; eng = r["eng"]
    dx, dy = cotangents(3, t["base_dx"], t["base_dy"])
    dxt = torch.from_numpy(dx).cuda()
    kw = dict(path="per_instance", P_bm=r["P_bm"], qp_many=True)
    a = eng.vjp_many(r["A_bm"], *r["pt"], dxt, None, **kw)
    assert eng.last_vjp_many_path == "many" and eng.last_vjp_kernel == "ce_vjp_qp_many"
    b = eng.vjp_many(r["A_bm"], *r["pt"], dxt, torch.zeros(dy.shape, dtype=torch.float64, device="cuda"), **kw)
    assert len(a) == len(b) == 4 and all(torch.equal(u, v) for u, v in zip(a, b)) and a[3].abs().max() > 0


def test_a_flagged_instance_keeps_status_four_for_every_cotangent():
    """test_gpu_jvp_qp_many.py's duplicated equality row on the small mixed shape: every second instance"""
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
    dx, dy = (torch.from_numpy(a).cuda() for a in cotangents(K, t["base_dx"], t["base_dy"]))
    pt = tuple(torch.from_numpy(ref[k]).cuda() for k in "xys")
    out = eng.vjp_many(A_bm, *pt, dx, dy, path="per_instance", P_bm=P_bm, qp_many=True)
    assert eng.last_vjp_many_path == "many"
    loop = eng.vjp_many(A_bm, *pt, dx, dy, path="per_instance", P_bm=P_bm)
    torch.cuda.synchronize()
    st = out[2].cpu().numpy()
    for k in range(K):
        assert (st[k][deg] == 4).all() and (st[k][~deg] == 0).all(), (k, st[k])
    keep = torch.from_numpy(~deg).cuda()
    assert (loop[2][:, keep] == 0).all()
    for i in (0, 1, 3):
        assert torch.isfinite(out[i]).all()
        e = ((out[i] - loop[i]).abs().amax(dim=2) / (1 + loop[i].abs().amax(dim=2)))[:, keep].max().item()
        assert e < 1e-6, (i, e)


def test_the_entries_refuse_the_other_kind_of_template_and_strided_rows():
    from test_gpu_jvp import _engine
    L = _lib.lib()
    t = _shape("small_mixed")
    r = t["r"]; eng = r["eng"]
    K, B = 2, t["B"]
    f64 = dict(dtype=torch.float64, device="cuda")
    # ce_vjp_many keeps refusing a QP-native template
    z = torch.zeros((K, B, max(eng.n + 1, eng.m, eng.nnz_aug, eng.nnz_p)), **f64); st = torch.zeros((K, B), dtype=torch.int32, device="cuda")
    rc = L.ce_vjp_many(eng._h, B, K, r["A_bm"].data_ptr(), eng.nnz_aug, r["q_t"].data_ptr(), r["q_t"].stride(0), r["q_t"].stride(1), *(u.data_ptr() for u in r["pt"]),
                       z.data_ptr(), None, z.data_ptr(), z.data_ptr(), st.data_ptr(), None)
    assert rc == -2 and b"quadratic objective" in L.ce_last_error()
    # non-contiguous A rows: CE_E_BADARG
    rc = L.ce_vjp_qp_many(eng._h, B, K, r["A_bm"].data_ptr(), eng.nnz_aug + 1, r["P_bm"].data_ptr(), *(u.data_ptr() for u in r["pt"]), z.data_ptr(), None,
                          z.data_ptr(), z.data_ptr(), z.data_ptr(), st.data_ptr(), None)
    assert rc == -1 and b"ce_vjp_qp_many" in L.ce_last_error() and b"contiguous" in L.ce_last_error()
    # ce_vjp_qp_many on a linear-objective template: CE_E_UNSUPPORTED, the reason named
    e = _engine(P.dense_template(12, {"z": 2, "l": 6, "q": [4, 5]}))
    assert L.ce_qp_native(e._h) == 0 and L.ce_vjp_qp_many_variant(e._h) == -1
    z = torch.zeros((K, 3, max(e.n + 1, e.m, e.nnz_aug, 2)), **f64); st = torch.zeros((K, 3), dtype=torch.int32, device="cuda")
    rc = L.ce_vjp_qp_many(e._h, 3, K, z.data_ptr(), e.nnz_aug, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None,
                          z.data_ptr(), z.data_ptr(), z.data_ptr(), st.data_ptr(), None)
    assert rc == -2 and b"ce_vjp_qp_many" in L.ce_last_error() and b"ce_qp_native" in L.ce_last_error(), (rc, L.ce_last_error())
    torch.cuda.synchronize()

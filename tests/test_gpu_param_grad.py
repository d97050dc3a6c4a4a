"""Parameter gradients straight from the adjoint's factors at the engine level (ConeEngine.vjp_many_params / vjp_params, csrc/ce_param_grad.h), at planted KKT
points of ns_edge_kit: no solve.

Reference: today's route on the SAME engine -- vjp_many, then the two transposed-map products of the frontend (_spmm_bm) -- which test_gpu_ns_many_edges.py pins
to the oracle's dense adjoint.  Required of the new route, per (shape, B, K, map):
  * torch.equal with the reference on every parameter row with exactly one map entry in total (the entry is rounded as the dA entry, then multiplied);
  * on every other row |g - g_ref| <= t 2^-52 sum |val_e entry_e|, t the row's term count, the sum in np.longdouble from the reference's dA, dq.  Derived: each
    route adds t products rounded once (relative 2^-53 each) in t - 1 (here: t, from a zero sum) additions of relative error 2^-53, so each is within
    t 2^-53 sum |terms| of the exact sum to first order, whatever its order of summation; the two differ by at most twice that;
  * exact zeros for the zero cotangent and for an empty row; the repeated cotangent equals the first; dq and adj_status equal vjp_many's.
Shapes: the kit's smallest structure shapes (n = 1, 2, 3, z = n, no active row -- the plain kind of that shape is singular: every instance is re-solved by LSQR,
so the record mode of the LSQR walk is exercised on a whole batch) and both sides of the column-rule edge n = 28 / 29.  B = 1 and 37 (the tile of 16 pairs: a
partial tile, three tiles and a tile that spans two cotangents), K = 1 and 4 (two Gaussian draws, zero, the first again).
Maps, synthetic: every entry its own parameter with a constant column present in both maps; b / c columns only; Ptot = 1 with one parameter on every A entry (a
long row) and an empty constant row; 2300 rows (more than one slab of the kernel) of 0 - 3 entries drawn from both maps."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ns_edge_kit as K
import plan_kit as pk
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from cvxpylayers_amd.interfaces.param_grad import ComposedMaps
from kit import TIGHT_LSQR
from test_gpu_ns_mode_edges import _device, _engine

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
KC, ZERO_AT, REPEAT_AT = 4, 2, 3
BIG = 37
SHAPES = {
    "n1": K.STRUCTURE["n1"]["plain"],
    "n2_one_q3": K.STRUCTURE["n2_one_q3"]["plain"],
    "n3": K.STRUCTURE["n3"]["plain"],
    "z_is_n6": K.STRUCTURE["z_is_n6"]["plain"],
    "no_active_row": ("plain",) + K.STRUCTURE["no_active_row"]["qp"][1:],
    "plain_n[28]": pk.NS_FAMILIES["plain_n"][2](28),
    "plain_n[29]": pk.NS_FAMILIES["plain_n"][2](29),
}
PLANT_ARGS = {"no_active_row": dict(active=0)}
_CASES: dict = {}


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for e in pk.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)


def synthetic_maps(tpl, seed):
    """{name: (A_mapT (rows, nnz_aug), q_mapT (rows, n + 1))} as scipy CSR; values Gaussian, never zero"""
    rng = np.random.default_rng(seed)
    nnz, n = tpl.nnz_aug, tpl.n
    nnzA = int(tpl.indptr[n])
    val = lambda k: rng.standard_normal(k) + np.sign(rng.standard_normal(k)) * 0.1
    out = {}
    # every entry its own parameter; the last row is the constant column, present in both maps
    rows = nnz + n + 1 + 1
    ck = rng.choice(nnz, size=min(nnz, 3), replace=False); cj = rng.choice(n + 1, size=min(n + 1, 2), replace=False)
    A = sp.csr_array((np.concatenate([val(nnz), val(ck.size)]), (np.concatenate([np.arange(nnz), np.full(ck.size, rows - 1)]), np.concatenate([np.arange(nnz), ck]))), shape=(rows, nnz))
    q = sp.csr_array((np.concatenate([val(n + 1), val(cj.size)]), (np.concatenate([nnz + np.arange(n + 1), np.full(cj.size, rows - 1)]), np.concatenate([np.arange(n + 1), cj]))), shape=(rows, n + 1))
    out["own"] = (A, q)
    # b / c columns only: a parameter per b entry and per c entry, a constant column on b
    nb = nnz - nnzA
    rows = nb + n + 1
    A = sp.csr_array((np.concatenate([val(nb), val(nb)]), (np.concatenate([np.arange(nb), np.full(nb, rows - 1)]), np.concatenate([nnzA + np.arange(nb)] * 2))), shape=(rows, nnz))
    q = sp.csr_array((val(n), (nb + np.arange(n), np.arange(n))), shape=(rows, n + 1))
    out["bc"] = (A, q)
    # Ptot = 1: one parameter on every A entry (b column included); the constant row is empty
    A = sp.csr_array((val(nnz), (np.zeros(nnz, int), np.arange(nnz))), shape=(2, nnz))
    q = sp.csr_array((2, n + 1))
    out["scalar"] = (A, q)
    # more rows than one slab of the kernel (2048): 0 - 3 entries per row, drawn from both maps
    rows = 2300
    cnt = rng.integers(0, 4, rows); cnt[7] = 0; cnt[2050] = 1
    rr = np.repeat(np.arange(rows), cnt)
    inA = rng.random(rr.size) < 0.7
    # (distinct columns per row are not required of a CSR map in general, but scipy sums duplicates: draw, then let it)
    A = sp.csr_array((val(int(inA.sum())), (rr[inA], rng.integers(0, nnz, int(inA.sum())))), shape=(rows, nnz))
    q = sp.csr_array((val(int((~inA).sum())), (rr[~inA], rng.integers(0, n + 1, int((~inA).sum())))), shape=(rows, n + 1))
    A.sum_duplicates(); q.sum_duplicates()
    out["many_rows"] = (A, q)
    return out


def case(name):
    """engine, planted point at B = 37, device data, cotangents, maps of a shape: built once"""
    if name not in _CASES:
        shape = SHAPES[name]
        pt = K.plant(shape, B=BIG, seed=5, **PLANT_ARGS.get(name, {}))
        tpl, eng = _engine(shape)
        assert _lib.lib().ce_vjp_many_variant(eng._h) >= 0 and eng.param_grad_variant == _lib.lib().ce_vjp_many_variant(eng._h), name
        dv = _device(pt, tpl, shape)
        rng = np.random.default_rng(77)
        xb = np.zeros((KC,) + pt["x"].shape); yb = np.zeros((KC,) + pt["y"].shape)
        for k in (0, 1):
            xb[k] = rng.standard_normal(pt["x"].shape); yb[k] = rng.standard_normal(pt["y"].shape)
        xb[REPEAT_AT], yb[REPEAT_AT] = xb[0], yb[0]
        maps = {}
        for mname, (A, q) in synthetic_maps(tpl, seed=3).items():
            from cvxpylayers_amd.torch.cvxpylayer import _DeviceCSR
            cm = ComposedMaps(A, q, tpl.indices, tpl.indptr, tpl.n, tpl.m)
            maps[mname] = dict(A=sp.csr_array(A), q=sp.csr_array(q), cm=cm, dA=_DeviceCSR(A), dq=_DeviceCSR(q))
        _CASES[name] = dict(pt=pt, tpl=tpl, eng=eng, dv=dv, xb=xb, yb=yb, maps=maps)
    return _CASES[name]


def reference(eng, dv, x, y, s, dx, dy, mp):
    """today's route: vjp_many, then the two transposed-map products; (g, dA, dq, adj)"""
    from cvxpylayers_amd.torch.cvxpylayer import _spmm_bm
    dA, dq, adj = eng.vjp_many(dv["A_bm"], x, y, s, dx, dy, path="per_instance", lsqr=TIGHT_LSQR, q_eval=dv["q_t"])
    assert eng.last_vjp_kernel == "ce_vjp_many"
    Kc, B = dA.shape[:2]
    fA, fq = mp["dA"].on(dA.device)[0], mp["dq"].on(dA.device)[0]          # (the maps are handed over transposed already: their forward product is the transposed map's)
    g = torch.zeros((Kc * B, mp["A"].shape[0]), dtype=torch.float64, device=dA.device)
    _spmm_bm(fA, dA.view(Kc * B, -1), out=g)
    _spmm_bm(fq, dq.view(Kc * B, -1), out=g)
    return g.view(Kc, B, -1), dA, dq, adj


def bound_of(mp, dA, dq):
    """(terms per row, t 2^-52 sum |val entry| per (k, b, row)) in np.longdouble from the reference's dA, dq"""
    Ld = np.longdouble
    absA, absq = abs(mp["A"]), abs(mp["q"])
    t = np.diff(mp["A"].indptr) + np.diff(mp["q"].indptr)
    Kc, B = dA.shape[:2]
    S = np.zeros((Kc * B, t.size), dtype=Ld)
    a, q = np.abs(dA.reshape(Kc * B, -1)).astype(Ld), np.abs(dq.reshape(Kc * B, -1)).astype(Ld)
    for M, v in ((absA.tocoo(), a), (absq.tocoo(), q)):
        for r, c, w in zip(M.row, M.col, M.data):
            S[:, r] += Ld(w) * v[:, c]
    return t, (t.astype(Ld) * Ld(U) * S).reshape(Kc, B, -1)


def compare(tag, g, g_ref, dA, dq, mp):
    t, bound = bound_of(mp, dA, dq)
    single = t == 1
    assert np.array_equal(g[:, :, single], g_ref[:, :, single]), f"{tag}: a row with one map entry differs from the dA route: max {np.abs(g[:, :, single] - g_ref[:, :, single]).max():.3e}"
    err = np.abs(g.astype(np.longdouble) - g_ref.astype(np.longdouble))
    over = err > bound
    worst = float((err / np.where(bound > 0, bound, 1)).max())
    print(f"{tag}: rows {t.size} (single {int(single.sum())}, empty {int((t == 0).sum())}, longest {int(t.max())}); max error / bound {worst:.3f}")
    assert not over.any(), f"{tag}: {int(over.sum())} entries beyond t 2^-52 sum |val entry| (worst ratio {worst:.3f})"
    assert (g[:, :, t == 0] == 0.0).all(), f"{tag}: an empty row is not exactly zero"
    return t


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("B", [1, BIG])
@pytest.mark.parametrize("Kc", [1, KC])
def test_param_grad_equals_the_dA_route(name, B, Kc):
    c = case(name)
    pt, eng, dv = c["pt"], c["eng"], c["dv"]
    dvB = dict(A_bm=dv["A_bm"][:B].contiguous(), q_t=dv["q_t"][:, :B].contiguous())
    x, y, s = (torch.from_numpy(np.ascontiguousarray(pt[k][:B])).cuda() for k in "xys")
    dx, dy = (torch.from_numpy(np.ascontiguousarray(a[:Kc, :B])).cuda() for a in (c["xb"], c["yb"]))
    for mname, mp in c["maps"].items():
        tag = f"{name} B={B} K={Kc} {mname}"
        g_ref, dA, dq_ref, adj_ref = reference(eng, dvB, x, y, s, dx, dy, mp)
        g, dq, adj = eng.vjp_many_params(dvB["A_bm"], x, y, s, dx, dy, mp["cm"], lsqr=TIGHT_LSQR, q_eval=dvB["q_t"])
        assert eng.last_vjp_many_path == "many_params" and eng.last_vjp_kernel == "ce_vjp_many_params", tag
        torch.cuda.synchronize()
        assert torch.equal(dq, dq_ref) and torch.equal(adj, adj_ref), f"{tag}: dq / adj_status differ from vjp_many's"
        gn, grn, dAn, dqn = (a.cpu().numpy() for a in (g, g_ref, dA, dq_ref))
        compare(tag, gn, grn, dAn, dqn, mp)
        if Kc == KC:
            assert (gn[ZERO_AT] == 0.0).all(), f"{tag}: the zero cotangent does not give exact zeros"
            assert np.array_equal(gn[REPEAT_AT], gn[0]), f"{tag}: the repeated cotangent differs from the first"
        else:
            # one cotangent on the single-cotangent kernel: vjp_params against vjp + the two products (flagged instances: the row the re-solve wrote is read back)
            from cvxpylayers_amd.torch.cvxpylayer import _spmm_bm
            dA1, dq1, adj1 = eng.vjp(dvB["A_bm"], x, y, s, dx[0], dy[0], path="per_instance", lsqr=TIGHT_LSQR, q_eval=dvB["q_t"])
            g1_ref = torch.zeros((B, mp["cm"].rows), dtype=torch.float64, device=x.device)
            _spmm_bm(mp["dA"].on(x.device)[0], dA1.t().contiguous(), out=g1_ref)
            _spmm_bm(mp["dq"].on(x.device)[0], dq1.t().contiguous(), out=g1_ref)
            g1, dq1p, adj1p = eng.vjp_params(dvB["A_bm"], x, y, s, dx[0], dy[0], mp["cm"], lsqr=TIGHT_LSQR, q_eval=dvB["q_t"])
            torch.cuda.synchronize()
            assert torch.equal(dq1p, dq1) and torch.equal(adj1p, adj1), f"{tag}: vjp_params: dq / adj_status differ from vjp's"
            compare(tag + " vjp_params", g1.cpu().numpy()[None], g1_ref.cpu().numpy()[None], dA1.t().cpu().numpy()[None], dq1.t().cpu().numpy()[None], mp)


def test_flagged_instance_goes_through_the_record_mode_of_the_lsqr_walk():
    """one instance made rank deficient by a duplicated equality row (tests/test_gpu_ns_adjoint.py builds it so): status 4 | 8 for every k, g within the bound of the
    dA route (the same LSQR solve, the same entry formula), and r_tau != 0 there: the b-column and dc terms are exercised.  At a planted point (no solve)."""
    shape = ("plain", 12, {"z": 4, "l": 8, "q": [5]}, ("bd",))
    B = 5
    pt = K.plant(shape, B=B, seed=11)
    A, b, c = pt["A"].copy(), pt["b"].copy(), pt["c"].copy()
    deg = 3
    # duplicate equality row 0 into row 2 and keep the point a KKT point: b_2 = a_0 . x + s_2, c = -A^T y
    A[deg, 2, :] = A[deg, 0, :]
    b[deg] = A[deg] @ pt["x"][deg] + pt["s"][deg]
    c[deg] = -A[deg].T @ pt["y"][deg]
    tpl, eng = _engine(shape)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    dv = dict(A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(), q_t=torch.from_numpy(q_eval).cuda())
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    rng = np.random.default_rng(19)
    xb = np.zeros((KC, B, pt["n"])); yb = np.zeros((KC, B, pt["m"]))
    for k in (0, 1):
        xb[k] = rng.standard_normal(xb[k].shape); yb[k] = rng.standard_normal(yb[k].shape)
    xb[REPEAT_AT], yb[REPEAT_AT] = xb[0], yb[0]
    dx, dy = torch.from_numpy(xb).cuda(), torch.from_numpy(yb).cuda()
    from cvxpylayers_amd.torch.cvxpylayer import _DeviceCSR
    for mname, (Am, qm) in synthetic_maps(tpl, seed=4).items():
        mp = dict(A=sp.csr_array(Am), q=sp.csr_array(qm), cm=ComposedMaps(Am, qm, tpl.indices, tpl.indptr, tpl.n, tpl.m), dA=_DeviceCSR(Am), dq=_DeviceCSR(qm))
        g_ref, dA, dq_ref, adj_ref = reference(eng, dv, x, y, s, dx, dy, mp)
        g, dq, adj = eng.vjp_many_params(dv["A_bm"], x, y, s, dx, dy, mp["cm"], lsqr=TIGHT_LSQR, q_eval=dv["q_t"])
        torch.cuda.synchronize()
        a = adj.cpu().numpy()
        assert (a[:, deg] == 12).all() and (np.delete(a, deg, axis=1) == 0).all(), a
        assert torch.equal(dq, dq_ref) and torch.equal(adj, adj_ref)
        gn, grn, dAn, dqn = (t.cpu().numpy() for t in (g, g_ref, dA, dq_ref))
        compare(f"flagged {mname}", gn, grn, dAn, dqn, mp)
        # r_tau is not observable from (dA, db, dc) -- adding a multiple of (x, y, 1) to r leaves them unchanged -- so it is read where it is stored: the records
        rec = eng.param_grad_records(KC, B).cpu().numpy()
        m, n = pt["m"], pt["n"]
        rt = rec[:, :, m]
        assert (np.delete(rt, deg, axis=1) == 0.0).all(), "the elimination pins r_tau to 0"
        assert (rt[[0, 1, REPEAT_AT], deg] != 0.0).all() and rt[ZERO_AT, deg] == 0.0, rt[:, deg]
        # and the records are the factors of the outputs: dc = x r_tau - r_x (one fma in both kernels)
        want_dq = pt["x"][None] * rt[:, :, None] - rec[:, :, m + 1:]
        assert np.abs(want_dq - dqn[:, :, :n]).max() <= 4 * U * (np.abs(pt["x"][None] * rt[:, :, None]) + np.abs(rec[:, :, m + 1:])).max()
        print(f"flagged {mname}: r_tau of the flagged instance per cotangent {rt[:, deg]}")


@pytest.mark.parametrize("kind", ["psd", "qp"])
def test_unserved_handles_are_refused_and_write_nothing(kind):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    n = 4
    cones = {"z": 1, "l": 3, "q": [3], "s": [2]} if kind == "psd" else {"z": 1, "l": 3, "q": [3]}
    tpl = P.dense_template(n, cones)
    eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0), p_structure=pk.ns_pstruct("qp", n) if kind == "qp" else None)
    assert eng.param_grad_variant == -1 and _lib.lib().ce_vjp_many_variant(eng._h) == -1
    B, Kc = 3, 2
    A, q = synthetic_maps(tpl, seed=1)["bc"]
    cm = ComposedMaps(A, q, tpl.indices, tpl.indptr, tpl.n, tpl.m)
    f64 = dict(dtype=torch.float64, device="cuda")
    A_bm, q_t = torch.ones((B, tpl.nnz_aug), **f64), torch.ones((n + 1, B), **f64)
    x, y, s = torch.zeros((B, n), **f64), torch.zeros((B, tpl.m), **f64), torch.zeros((B, tpl.m), **f64)
    dx, dy = torch.ones((Kc, B, n), **f64), torch.ones((Kc, B, tpl.m), **f64)
    out = torch.full((Kc, B, cm.rows), 7.0, **f64)
    with pytest.raises(_lib.EngineError, match=r"code -2.*ce_vjp_many_params"):
        eng.vjp_many_params(A_bm, x, y, s, dx, dy, cm, q_eval=q_t, out=out)
    with pytest.raises(_lib.EngineError, match=r"code -2.*ce_vjp_params"):
        eng.vjp_params(A_bm, x, y, s, dx[0], dy[0], cm, q_eval=q_t)
    torch.cuda.synchronize()
    assert (out == 7.0).all()

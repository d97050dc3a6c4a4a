"""Parameter gradients straight from the adjoint's factors for the four other many-cotangent kinds, at the engine level: ConeEngine.vjp_many_params(qp_many= /
tri_many= / psd_many=) -> ce_vjp_qp_many_params, ce_vjp_tri_many_params, ce_vjp_psd_many_params, ce_vjp_psd_tri_many_params (k_backward_ns<..., MANY> of each kind in
record mode, k_param_grad behind it with its third entry kind, dP).

Reference: the dA route of the SAME engine -- vjp_many with the kind's flag, then the transposed-map products of the frontend (_spmm_bm) with the same synthetic
maps (test_gpu_param_grad.synthetic_maps; for a QP three P maps beside them: every P entry its own parameter, one scalar parameter on all of P -- a long row --, and
a parameter with entries in the A, q and P maps together).  Required of every (shape, B, K, map), as test_gpu_param_grad.py requires of the plain kind:
  * dq and adj_status torch.equal to the dA route's;
  * torch.equal on every row with exactly one map entry in total -- P rows included: ce_dP_entry (csrc/ce_dA_entry.h) is shared by the QP adjoint's epilogue and
    k_param_grad, with the bits ce_vjp_qp_many's dP had before (the one-triangle doubling is an exact factor 2 in the composed value);
  * |g - g_ref| <= t 2^-52 sum |val_e entry_e| elsewhere (test_gpu_param_grad.bound_of's derivation; a P entry counts as a term like every other);
  * exact zeros for the zero cotangent and for an empty row; the repeated cotangent equals the first.
Shapes: the kits' smallest (see SHAPES below), B = 1 and the kit's own B, K = 1 and 4 (two Gaussian draws, zero, the first again).  B = 1 with K = 4 is a partial
tile of 16 pairs that spans four cotangents; the kits' B (16, 32, 48) fill whole tiles.  The points are the oracle's (the kits' shared, cached solves).
Flagged instances: duplicated equality rows (TRI: 12 for every k, r_tau != 0 in the records), a planted stiff PSD block (4 | 8), a rank-deficient QP instance
(status 4: the dropped-variable answer of both routes), and a QP instance with more active rows than variables (neq > n: zero record, exact zeros in g).
Every test here fails on a tree without the feature: the keywords and entries do not exist there."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import psd_ns_kit as PK
import psd_tri_ns_kit as PTK
import qp_ns_kit as Q
import tri_ns_kit as TK
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from cvxpylayers_amd.interfaces.param_grad import ComposedMaps
from kit import TIGHT_LSQR
from test_gpu_jvp import _engine
from test_gpu_param_grad import bound_of, compare, synthetic_maps
from test_quad_objective import _p_values, _upper_structure

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
KC, ZERO_AT, REPEAT_AT = 4, 2, 3
# kind -> (kit, shapes, the keyword of vjp_many / vjp_many_params, the entries' names)
KINDS = {
    "tri": (TK, ("exp_small", "triples_only", "exp_pow_mixed"), "tri_many", "ce_vjp_tri_many", "ce_vjp_tri_many_params"),
    "psd": (PK, ("psd_small", "psd_only", "psd_mixed"), "psd_many", "ce_vjp_psd_many", "ce_vjp_psd_many_params"),
    "psd_tri": (PTK, ("mix_small", "psd_tri_only", "mix_all"), "psd_many", "ce_vjp_psd_tri_many", "ce_vjp_psd_tri_many_params"),
}
QP_CASES = {"equality_qp": ("equality_qp", "upper"), "square_equalities": ("square_equalities", "upper"),
            "small_mixed_full": ("small_mixed", "full"), "small_mixed_upper": ("small_mixed", "upper")}
CONE_CASES = [(kind, name) for kind, v in KINDS.items() for name in v[1]]
_CASES: dict = {}


def _structure_rows_cols(struct):
    idx, ptr, _ = struct
    return np.asarray(idx, dtype=np.int64), np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)).astype(np.int64)


def p_maps(tpl, nnz_p, seed):
    """{name: (A_mapT, q_mapT, P_mapT)} for a QP: the three P maps the feature was specified with, each beside A / q maps of the same row count"""
    rng = np.random.default_rng(seed)
    nnz, n = tpl.nnz_aug, tpl.n
    val = lambda k: rng.standard_normal(k) + np.sign(rng.standard_normal(k)) * 0.1
    out = {}
    # every P entry its own parameter (one-entry rows: the bits of the dA route's dP); the rows behind them hold one A entry and one q entry each
    rows = nnz_p + 2
    out["p_own"] = (sp.csr_array((val(1), ([nnz_p], [nnz // 2])), shape=(rows, nnz)), sp.csr_array((val(1), ([nnz_p + 1], [n // 2])), shape=(rows, n + 1)),
                    sp.csr_array((val(nnz_p), (np.arange(nnz_p), np.arange(nnz_p))), shape=(rows, nnz_p)))
    # one scalar parameter on all of P (a long row where nnz_p > 32), an empty row behind it
    out["p_scalar"] = (sp.csr_array((2, nnz)), sp.csr_array((2, n + 1)), sp.csr_array((val(nnz_p), (np.zeros(nnz_p, int), np.arange(nnz_p))), shape=(2, nnz_p)))
    # parameters with entries in the A, q and P maps together: row r takes two A entries, one q entry and two P entries
    rows = 5
    pick = lambda cnt, hi: np.concatenate([rng.choice(hi, size=min(cnt, hi), replace=False) for _ in range(rows)])
    rep = lambda cnt, hi: np.repeat(np.arange(rows), min(cnt, hi))
    out["p_mixed"] = (sp.csr_array((val(rep(2, nnz).size), (rep(2, nnz), pick(2, nnz))), shape=(rows, nnz)),
                      sp.csr_array((val(rep(1, n + 1).size), (rep(1, n + 1), pick(1, n + 1))), shape=(rows, n + 1)),
                      sp.csr_array((val(rep(2, nnz_p).size), (rep(2, nnz_p), pick(2, nnz_p))), shape=(rows, nnz_p)))
    return out


def _maps_of(tpl, struct=None, p_tri=False, seed=3):
    from cvxpylayers_amd.torch.cvxpylayer import _DeviceCSR
    maps = {}
    for mname, (A, q) in synthetic_maps(tpl, seed=seed).items():
        maps[mname] = dict(A=sp.csr_array(A), q=sp.csr_array(q), cm=ComposedMaps(A, q, tpl.indices, tpl.indptr, tpl.n, tpl.m), dA=_DeviceCSR(A), dq=_DeviceCSR(q))
    if struct is not None:
        prow, pcol = _structure_rows_cols(struct)
        for mname, (A, q, Pm) in p_maps(tpl, prow.size, seed + 1).items():
            cm = ComposedMaps(A, q, tpl.indices, tpl.indptr, tpl.n, tpl.m, Pm, prow, pcol, p_tri)
            maps[mname] = dict(A=sp.csr_array(A), q=sp.csr_array(q), P=sp.csr_array(Pm), cm=cm, dA=_DeviceCSR(A), dq=_DeviceCSR(q), dP=_DeviceCSR(Pm))
    return maps


def _cotangents(x, y, seed=77):
    rng = np.random.default_rng(seed)
    xb = np.zeros((KC,) + x.shape); yb = np.zeros((KC,) + y.shape)
    for k in (0, 1):
        xb[k] = rng.standard_normal(x.shape); yb[k] = rng.standard_normal(y.shape)
    xb[REPEAT_AT], yb[REPEAT_AT] = xb[0], yb[0]
    return xb, yb


def cone_case(kind, name):
    """engine, the kit's oracle point, device data, cotangents and maps of a shape: built once, shared, not changed"""
    key = (kind, name)
    if key not in _CASES:
        kit = KINDS[kind][0]
        n, cones, A, b, c, ref = kit.problem(name)
        tpl = P.dense_template(n, cones)
        A_eval, q_eval = tpl.values_from_dense(A, b, c)
        xb, yb = _cotangents(ref["x"], ref["y"])
        _CASES[key] = dict(tpl=tpl, eng=_engine(tpl), A=A, b=b, c=c, cones=cones, ref=ref, A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(),
                           q_t=torch.from_numpy(q_eval).cuda(), pt=tuple(ref[k] for k in "xys"), xb=xb, yb=yb, maps=_maps_of(tpl), P_bm=None, flag=KINDS[kind][2],
                           kernel=KINDS[kind][3], entry=KINDS[kind][4])
    return _CASES[key]


def qp_case(cname):
    key = ("qp", cname)
    if key not in _CASES:
        from oracle import oracle
        name, which = QP_CASES[cname]
        n, cones, A, b, c, Pm = Q.instance(name)
        tpl = P.dense_template(n, cones)
        struct = Q.full_structure(n) if which == "full" else _upper_structure(n)
        ref = oracle.solve_batch(A, b, c, cones, P=Pm, eps=1e-10, max_iters=200000)
        A_bm, q_t, P_bm = Q.device_values(tpl, A, b, c, Pm, struct)
        xb, yb = _cotangents(ref["x"], ref["y"])
        eng = Q.qp_engine(tpl, struct)
        assert _lib.lib().ce_vjp_qp_many_variant(eng._h) >= 0, cname
        _CASES[key] = dict(tpl=tpl, eng=eng, A=A, b=b, c=c, Pm=Pm, cones=cones, ref=ref, struct=struct, A_bm=A_bm, q_t=q_t, P_bm=P_bm, pt=tuple(ref[k] for k in "xys"),
                           xb=xb, yb=yb, maps=_maps_of(tpl, struct, p_tri=which == "upper"), flag="qp_many", kernel="ce_vjp_qp_many", entry="ce_vjp_qp_many_params")
    return _CASES[key]


def both_routes(c, mp, A_bm, q_t, P_bm, x, y, s, dx, dy):
    """(g, dq, adj) of the factor route and (g_ref, dA, dq + dP side by side, adj) of the dA route; mp_ext: the map with P's columns appended to q's, so that
    test_gpu_param_grad.bound_of / compare count a P entry as a term like every other"""
    from cvxpylayers_amd.torch.cvxpylayer import _spmm_bm
    eng = c["eng"]
    kw = dict(P_bm=P_bm) if P_bm is not None else dict(lsqr=TIGHT_LSQR, q_eval=q_t)
    ref = eng.vjp_many(A_bm, x, y, s, dx, dy, path="per_instance", **kw, **{c["flag"]: True})
    assert eng.last_vjp_many_path == "many" and eng.last_vjp_kernel == c["kernel"], (eng.last_vjp_many_path, eng.last_vjp_kernel)
    dA, dq_ref, adj_ref = ref[:3]
    Kc, B = dA.shape[:2]
    g_ref = torch.zeros((Kc * B, mp["cm"].rows), dtype=torch.float64, device=dA.device)
    _spmm_bm(mp["dA"].on(dA.device)[0], dA.view(Kc * B, -1), out=g_ref)
    _spmm_bm(mp["dq"].on(dA.device)[0], dq_ref.view(Kc * B, -1), out=g_ref)
    ext, mp_ext = dq_ref, mp
    if "P" in mp:
        _spmm_bm(mp["dP"].on(dA.device)[0], ref[3].view(Kc * B, -1), out=g_ref)
        ext = torch.cat([dq_ref, ref[3]], dim=2)
        mp_ext = dict(A=mp["A"], q=sp.csr_array(sp.hstack([mp["q"], mp["P"]])))
    g, dq, adj = eng.vjp_many_params(A_bm, x, y, s, dx, dy, mp["cm"], **kw, **{c["flag"]: True})
    assert eng.last_vjp_many_path == "many_params" and eng.last_vjp_kernel == c["entry"], (eng.last_vjp_many_path, eng.last_vjp_kernel)
    torch.cuda.synchronize()
    return (g, dq, adj), (g_ref.view(Kc, B, -1), dA, dq_ref, adj_ref, ext), mp_ext


def check(tag, c, B, Kc, A_bm=None, pt=None):
    sl = lambda a: torch.from_numpy(np.ascontiguousarray(a[:B])).cuda()
    x, y, s = (sl(a) for a in (pt or c["pt"]))
    A_bm = (c["A_bm"] if A_bm is None else A_bm)[:B].contiguous()
    q_t = c["q_t"][:, :B].contiguous()
    P_bm = None if c["P_bm"] is None else c["P_bm"][:B].contiguous()
    dx, dy = (torch.from_numpy(np.ascontiguousarray(a[:Kc, :B])).cuda() for a in (c["xb"], c["yb"]))
    adj_out = None
    for mname, mp in c["maps"].items():
        t = f"{tag} B={B} K={Kc} {mname}"
        (g, dq, adj), (g_ref, dA, dq_ref, adj_ref, ext), mp_ext = both_routes(c, mp, A_bm, q_t, P_bm, x, y, s, dx, dy)
        assert torch.equal(dq, dq_ref) and torch.equal(adj, adj_ref), f"{t}: dq / adj_status differ from the dA route's"
        gn, grn = g.cpu().numpy(), g_ref.cpu().numpy()
        compare(t, gn, grn, dA.cpu().numpy(), ext.cpu().numpy(), mp_ext)
        if Kc == KC:
            assert (gn[ZERO_AT] == 0.0).all(), f"{t}: the zero cotangent does not give exact zeros"
            assert np.array_equal(gn[REPEAT_AT], gn[0]), f"{t}: the repeated cotangent differs from the first"
        adj_out = adj.cpu().numpy()
    return adj_out


@pytest.mark.parametrize("Kc", [1, KC])
@pytest.mark.parametrize("whole", [False, True], ids=["B1", "kitB"])
@pytest.mark.parametrize("kind,name", CONE_CASES)
def test_cone_kinds_equal_the_dA_route(kind, name, whole, Kc):
    c = cone_case(kind, name)
    L = _lib.lib()
    served = dict(tri=L.ce_vjp_tri_many_variant, psd=L.ce_vjp_psd_many_variant, psd_tri=L.ce_vjp_psd_tri_many_variant)[kind](c["eng"]._h)
    assert served >= 0 and c["eng"].param_grad_variant == -1, (kind, name)          # (the plain entries keep refusing this handle)
    check(f"{kind} {name}", c, c["A"].shape[0] if whole else 1, Kc)


@pytest.mark.parametrize("Kc", [1, KC])
@pytest.mark.parametrize("whole", [False, True], ids=["B1", "kitB"])
@pytest.mark.parametrize("cname", list(QP_CASES))
def test_qp_kind_equals_the_dA_route_dP_included(cname, whole, Kc):
    c = qp_case(cname)
    nnz_p = c["P_bm"].shape[1]
    if cname == "small_mixed_full":
        assert nnz_p == 144 and np.diff(c["maps"]["p_scalar"]["cm"].ptr).max() == 144          # the long-row path over P entries
    if cname == "small_mixed_upper":
        cm = c["maps"]["p_own"]["cm"]
        prow, pcol = _structure_rows_cols(c["struct"])
        off = prow != pcol
        assert off.any() and np.array_equal(cm.val[:nnz_p][off], 2.0 * c["maps"]["p_own"]["P"].data[off])          # the doubling stands in the composed value
    check(f"qp {cname}", c, c["A"].shape[0] if whole else 1, Kc)


def test_tri_duplicated_equality_rows_go_through_the_record_mode_of_the_lsqr_walk():
    """test_gpu_vjp_tri_many.py's construction on exp_pow_mixed: status 12 for every k on the degenerate instances, g within the bound of the dA route (the same LSQR
    solve, the same entry formulas), and r_tau != 0 there, read where it is stored: the records"""
    from oracle import oracle
    n, cones, B, seed, _ = TK.SHAPES["exp_pow_mixed"]
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
    xb, yb = _cotangents(ref["x"], ref["y"], seed=19)
    case = dict(tpl=tpl, eng=_engine(tpl), A=A, A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(), q_t=torch.from_numpy(q_eval).cuda(),
                pt=tuple(ref[k] for k in "xys"), xb=xb, yb=yb, maps=_maps_of(tpl, seed=4), P_bm=None, flag="tri_many", kernel="ce_vjp_tri_many", entry="ce_vjp_tri_many_params")
    Bk = A.shape[0]
    a = check("tri duplicated rows", case, Bk, KC)
    assert (a[:, deg] == 12).all() and (a[:, ~deg] == 0).all(), a
    rec = case["eng"].param_grad_records(KC, Bk).cpu().numpy()
    m = tpl.m
    assert rec.shape == (KC, Bk, m + 1 + n)
    rt = rec[:, :, m]
    assert (rt[:, ~deg] == 0.0).all(), "the elimination pins r_tau to 0"
    assert (rt[[0, 1, REPEAT_AT]][:, deg] != 0.0).all() and (rt[ZERO_AT][deg] == 0.0).all(), rt[:, deg]
    print(f"tri duplicated rows: r_tau of the first flagged instance per cotangent {rt[:, np.flatnonzero(deg)[0]]}")


def test_psd_planted_stiff_block_is_resolved_into_records():
    c = dict(cone_case("psd", "psd_mixed"))
    inst = 3
    y, s = PK.plant_stiff_block(c["ref"]["y"], c["ref"]["s"], c["cones"], inst)
    assert PK.block_states(y[inst] - s[inst], c["cones"])[1] < 1e-5
    a = check("psd stiff block", c, c["A"].shape[0], KC, pt=(c["ref"]["x"], y, s))
    assert (a[:, inst] == (4 | 8)).all(), a[:, inst]
    assert (np.delete(a, inst, axis=1) == 0).mean() >= 0.8


def test_qp_rank_deficient_instance_keeps_the_dropped_variable_answer():
    """test_gpu_vjp_qp_many.py's duplicated equality row on small_mixed, every second instance, at the case's point (the derivative system is linear algebra at the
    point given): status 4 for every k on both routes, never 4 | 8, g within the bound of the dA route's answer"""
    c = dict(qp_case("small_mixed_upper"))
    A = c["A"].copy()
    deg = np.arange(A.shape[0]) % 2 == 0
    A[deg, 1, :] = A[deg, 0, :]
    A_bm, _, _ = Q.device_values(c["tpl"], A, c["b"], c["c"], c["Pm"], c["struct"])
    a = check("qp rank deficient", c, A.shape[0], KC, A_bm=A_bm)
    assert (a[:, deg] == 4).all() and (a[:, ~deg] == 0).all(), a


def test_qp_instance_with_more_active_rows_than_variables_gets_a_zero_record():
    """small_mixed (n = 12, m = 17) with instance 5's dual point strictly inside every cone and s = 0: every row is active, neq = 17 > n -- rank deficient by
    counting.  The QP kind has no re-solve: status 4, zero record, exact zeros in g, dq and (on the dA route) dA and dP"""
    c = dict(qp_case("small_mixed_upper"))
    inst, cones = 5, c["cones"]
    x, y, s = (a.copy() for a in c["pt"])
    y[inst] = 1.0; s[inst] = 0.0
    r0 = cones["z"] + cones["l"]
    for q in cones["q"]:
        y[inst, r0] = 3.0 * np.sqrt(q); r0 += q          # (t > |z|: the interior of the second-order cone)
    B = c["A"].shape[0]
    a = check("qp neq > n", c, B, KC, pt=(x, y, s))
    assert (a[:, inst] == 4).all(), a[:, inst]
    eng, mp = c["eng"], c["maps"]["own"]
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    dx, dy = dev(c["xb"]), dev(c["yb"])
    dA, dq_ref, _, dP = eng.vjp_many(c["A_bm"], dev(x), dev(y), dev(s), dx, dy, path="per_instance", P_bm=c["P_bm"], qp_many=True)
    assert (dA[:, inst] == 0).all() and (dP[:, inst] == 0).all() and (dq_ref[:, inst] == 0).all() and (dA[0, inst - 1] != 0).any()
    g, dq, adj = eng.vjp_many_params(c["A_bm"], dev(x), dev(y), dev(s), dx, dy, mp["cm"], P_bm=c["P_bm"], qp_many=True)
    rec = eng.param_grad_records(KC, B)
    torch.cuda.synchronize()
    assert (rec[:, inst] == 0).all() and (g[:, inst] == 0).all() and (dq[:, inst] == 0).all()
    assert (rec[0, inst - 1] != 0).any() and (g[0, inst - 1] != 0).any()


def test_every_new_entry_refuses_a_handle_of_another_kind_and_writes_nothing():
    """each entry is served exactly where its kind's many-cotangent variant is >= 0: the engines of the four kinds and a plain one, every entry on every other handle"""
    L = _lib.lib()
    engines = {"tri": cone_case("tri", "exp_small"), "psd": cone_case("psd", "psd_small"), "psd_tri": cone_case("psd_tri", "mix_small"), "qp": qp_case("equality_qp")}
    ptpl = P.dense_template(4, {"z": 1, "l": 3, "q": [3]})
    engines["plain"] = dict(tpl=ptpl, eng=_engine(ptpl))
    assert engines["plain"]["eng"].param_grad_variant >= 0
    entries = {"tri": "ce_vjp_tri_many_params", "psd": "ce_vjp_psd_many_params", "psd_tri": "ce_vjp_psd_tri_many_params", "qp": "ce_vjp_qp_many_params"}
    f64 = dict(dtype=torch.float64, device="cuda")
    B, Kc = 3, 2
    for hk, c in engines.items():
        tpl, eng = c["tpl"], c["eng"]
        n, m = tpl.n, tpl.m
        A, q = synthetic_maps(tpl, seed=1)["bc"]
        cm = ComposedMaps(A, q, tpl.indices, tpl.indptr, n, m)
        ptr, code, kidx, val = cm.on(eng.device)
        A_bm, q_t = torch.ones((B, tpl.nnz_aug), **f64), torch.ones((n + 1, B), **f64)
        x, y, s = torch.zeros((B, n), **f64), torch.zeros((B, m), **f64), torch.zeros((B, m), **f64)
        dx, dy = torch.ones((Kc, B, n), **f64), torch.ones((Kc, B, m), **f64)
        P_bm = torch.ones((B, max(1, eng.nnz_p)), **f64)
        out, dq = torch.full((Kc, B, cm.rows), 7.0, **f64), torch.full((Kc, B, n + 1), 7.0, **f64)
        adj = torch.full((Kc, B), 7, dtype=torch.int32, device="cuda")
        _lib.check(L.ce_set_adjoint_resolve(eng._h, 1, 1e-12, 1e-12, 1e8, 100), "ce_set_adjoint_resolve"); eng._resolve_rule = None
        tail = (cm.rows, ptr.data_ptr(), code.data_ptr(), kidx.data_ptr(), val.data_ptr(), out.data_ptr(), dq.data_ptr(), adj.data_ptr(), None)
        for ek, entry in entries.items():
            if ek == hk:
                continue
            if ek == "qp":
                rc = L.ce_vjp_qp_many_params(eng._h, B, Kc, A_bm.data_ptr(), tpl.nnz_aug, P_bm.data_ptr(), x.data_ptr(), y.data_ptr(), s.data_ptr(), dx.data_ptr(), dy.data_ptr(), *tail)
            else:
                rc = getattr(L, entry)(eng._h, B, Kc, A_bm.data_ptr(), tpl.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                                       dx.data_ptr(), dy.data_ptr(), *tail)
            assert rc == -2 and entry.encode() in L.ce_last_error(), (hk, entry, rc, L.ce_last_error())          # CE_E_UNSUPPORTED, naming the entry
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (dq == 7.0).all() and (adj == 7).all(), hk
    # and through the binding: the keyword selects the entry, the library refuses
    c = engines["plain"]; tpl, eng = c["tpl"], c["eng"]
    A, q = synthetic_maps(tpl, seed=1)["bc"]
    cm = ComposedMaps(A, q, tpl.indices, tpl.indptr, tpl.n, tpl.m)
    A_bm, q_t = torch.ones((B, tpl.nnz_aug), **f64), torch.ones((tpl.n + 1, B), **f64)
    x, y, s = torch.zeros((B, tpl.n), **f64), torch.zeros((B, tpl.m), **f64), torch.zeros((B, tpl.m), **f64)
    out = torch.full((Kc, B, cm.rows), 7.0, **f64)
    for kw, entry in ((dict(tri_many=True), "ce_vjp_tri_many_params"), (dict(psd_many=True), "ce_vjp_psd_many_params")):
        with pytest.raises(_lib.EngineError, match=r"code -2.*" + entry):
            eng.vjp_many_params(A_bm, x, y, s, torch.ones((Kc, B, tpl.n), **f64), None, cm, q_eval=q_t, out=out, **kw)
    torch.cuda.synchronize()
    assert (out == 7.0).all()

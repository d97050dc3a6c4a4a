"""Every mode of the search-free elimination k_backward_ns at the edges of its three planners (csrc/ce_plan.h ns_variant / qp_ns_variant / tri_ns_variant) and at
the smallest shapes at which each part of its LDS layout exists (ns_edge_kit.STRUCTURE).

Shapes: both sides of every edge plan_kit.ns_edges finds on the host plan (the column rule, the three footprints going over LDS, the QP planner's own limits), B = 24
when n m <= 6000 and 8 above.  Points: planted KKT points (ns_edge_kit.plant; tests/test_ns_edge_kit.py proves every instance regular without a GPU).  At each shape
  * the library's plan equals the host plan on all three variant fields;
  * the forward derivative (ce_jvp, ce_jvp_qp) against the dense solve on EVERY instance: status-0 instances within 1e-5 maximum / 1e-8 median relative to
    1 + max |reference| with no LSQR iteration; flagged ones (4 | 8; QP: 4) re-solved under TIGHT_LSQR to the flagged bound of test_gpu_jvp_direct.py (median 1e-6,
    maximum 5e-3), QP finite; null tangents give exact zeros;
  * the adjoint (plain kind, ce_vjp with q_eval) against the oracle's dense elimination at the planted point within 1e-5, and the transpose identity between the two;
  * one Newton step (ce_refine, ce_refine_qp) from the planted point moved by 1e-6 relative: the returned point lies within ten times the distance at which the
    extended-precision dense step lands (plus the floor of _refine_floor), rho does not grow, a flagged instance keeps its point bit for bit;
  * on the first refused shape: CE_E_UNSUPPORTED at the C ABI with nothing written, the LSQR entry point behind ConeEngine.jvp, the point kept by ConeEngine.refine.
Ledger: every (row of CE_NS_VARIANTS, mode of csrc/ce_tu_ns.hip) must be reached by a compared call at a shape where >= 80 % of the instances have status 0."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

import ns_edge_kit as K
import plan_kit as pk
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_quad_objective import _p_values

pytestmark = pytest.mark.gpu

_DONE: dict = {}          # case name -> record (metrics and the ledger entries it reached)
MIN_REGULAR = 0.8
EPS = np.finfo(np.float64).eps


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for e in pk.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)


def ns_modes():
    """{mode struct name: (kind, call)} parsed from the three NS_MODES lists of csrc/ce_tu_ns.hip; call: "adjoint" | "jvp" | "refine" """
    src = open(os.path.join(pk.ROOT, "cvxpylayers_amd", "csrc", "ce_tu_ns.hip")).read()
    out = {}
    for line in re.findall(r"#define NS_MODES\(Y\)(.*)", src):
        for fwd, ref, qp, tri, name in re.findall(r"Y\((true|false), (true|false), (true|false), (true|false), (\w+)\)", line):
            kind = "qp" if qp == "true" else "tri" if tri == "true" else "plain"
            out[name] = (kind, "refine" if ref == "true" else "jvp" if fwd == "true" else "adjoint")
    return out


def ledger_entries():
    return [(row[0], name) for row in pk.variant_rows("CE_NS_VARIANTS") for name in ns_modes()]


def _mode_name(kind, call):
    (name,) = [nm for nm, kc in ns_modes().items() if kc == (kind, call)]
    return name


def _engine(shape):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    kind, n, cones, _ = shape
    tpl = P.dense_template(n, cones)
    return tpl, ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0), p_structure=pk.ns_pstruct(kind, n))


def _library_plan(eng):
    L = _lib.lib()
    return {"ns_variant": L.ce_adjoint_ns_variant(eng._h), "qp_ns_variant": L.ce_qp_ns_variant(eng._h), "tri_ns_variant": L.ce_tri_ns_variant(eng._h)}


def _assert_plans_agree(name, shape, eng):
    host = pk.host_ns_plan(shape)
    assert host is not None, name
    got = _library_plan(eng)
    assert got == {f: host[f] for f in pk.NS_FIELDS}, (name, got, host)
    plan = eng.plan()
    assert plan["ns_variant"] == host["ns_variant"] and plan["tri_ns_variant"] == host["tri_ns_variant"], (name, plan, host)
    return host


def _device(pt, tpl, shape):
    A_eval, q_eval = tpl.values_from_dense(pt["A"], pt["b"], pt["c"])
    d = dict(A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(), q_t=torch.from_numpy(q_eval).cuda(), P_bm=None)
    if pt["kind"] == "qp":
        ps = pk.ns_pstruct("qp", pt["n"])
        d["struct"] = (ps[0], ps[1], (pt["n"], pt["n"]))
        d["P_bm"] = torch.from_numpy(np.ascontiguousarray(_p_values(pt["Pm"], d["struct"]))).cuda()
    return d


def _rel(got, want):
    """per instance: max |got - want| / (1 + max |want|)"""
    return np.abs(got - want).max(axis=1) / (1 + np.abs(want).max(axis=1))


def _boundary(tpl, g, n):
    cols = np.repeat(np.arange(n + 1), np.diff(tpl.indptr))
    return np.stack([-g["dA"][:, i, j] if j < n else g["db"][:, i] for i, j in zip(tpl.indices, cols)])


def _refine_floor(pt, d_start):
    """What a step computed in plain double precision may add to the distance of the extended-precision reference (which solves with iterative refinement and
    lands at the rounding of its own output): the forward error eps cond(J) |step| of a backward-stable solve of the step -- |step| is the starting distance, cond(J)
    is known from the planted point -- and four roundings of the stored point, relative to 1 + max(|x*|, |v*|).  Nothing here is measured on the kernel."""
    scale = 1 + np.maximum(np.abs(pt["x"]).max(axis=1), np.abs(pt["v"]).max(axis=1))
    return EPS * K.regularity(pt)[0] * d_start + 4 * EPS * scale


def served_case(name, shape, resolve_only=False):
    """all checks at a shape its kind serves; the record.  resolve_only: ce_jvp is refused (the LSQR vectors do not fit), ce_refine is served and checked"""
    if name in _DONE:
        return _DONE[name]
    kind, n = shape[0], shape[1]
    pt = K.point(name, shape, **K.plant_args(name))
    cond, resid = K.regularity(pt)
    assert (cond <= 1e11).all() and (resid <= 1e-13).all(), (name, cond, resid)
    tpl, eng = _engine(shape)
    host = _assert_plans_agree(name, shape, eng)
    row = host[pk.NS_KIND_FIELD[kind]]
    assert row >= 0, (name, host)
    dv = _device(pt, tpl, shape)
    B, m = pt["x"].shape[0], pt["m"]
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    rec = dict(name=name, kind=kind, n=n, m=m, B=B, row=row, reached=[])
    tag = f"{name} ({kind}, n {n}, m {m}, B {B}, row {row})"
    qp = kind == "qp"

    # ---- the forward derivative
    t = K.tangents(pt)
    tA_eval, tq_eval = tpl.values_from_dense(*t[:3])
    tA_bm, tq = torch.from_numpy(tA_eval).cuda().t().contiguous(), torch.from_numpy(tq_eval).cuda()
    kw = dict(method="direct", P_bm=dv["P_bm"], tP_bm=torch.from_numpy(np.ascontiguousarray(_p_values(t[3], dv["struct"]))).cuda()) if qp else \
        dict(method="direct", path="per_instance", lsqr=TIGHT_LSQR, q_eval=dv["q_t"])
    st = None
    if resolve_only:
        rc, msg = _raw_jvp(eng, shape)
        assert rc == -2 and "re-solve" in msg, (tag, rc, msg)
    else:
        got = eng.jvp(dv["A_bm"], x, y, s, tA_bm, tq, **kw)
        assert eng.last_jvp_kernel == ("ce_jvp_qp" if qp else "ce_jvp"), (tag, eng.last_jvp_kernel)
        torch.cuda.synchronize()
        dx, dy, ds, st = (g.cpu().numpy() for g in got); its = eng.last_lsqr_iters.cpu().numpy()
        want = K.dense_jvp(pt, t)
        assert want[3].all(), tag          # no instance left out on the reference's account
        e = np.max([_rel(g, w) for g, w in zip((dx, dy, ds), want[:3])], axis=0)
        reg = st == 0
        fl = ~reg
        rec.update(jvp_share=float(reg.mean()), jvp_status=np.bincount(st).tolist())
        if reg.any():
            rec.update(jvp_max=float(e[reg].max()), jvp_median=float(np.median(e[reg])))
            print(f"{tag} jvp: regular share {reg.mean():.3f} status counts {np.bincount(st).tolist()} max {e[reg].max():.3e} median {np.median(e[reg]):.3e}")
            assert e[reg].max() < 1e-5 and np.median(e[reg]) < 1e-8, (tag, e[reg].max(), np.median(e[reg]))
            assert (its[reg] == 0).all(), (tag, its)
        if fl.any():          # flagged instances are not excused
            print(f"{tag} jvp: flagged {int(fl.sum())}: status {st[fl].tolist()} iterations {its[fl].tolist()} error {e[fl].tolist()}")
            if qp:
                assert (st[fl] == 4).all() and (its[fl] == 0).all(), (tag, st, its)
                assert all(np.isfinite(g[fl]).all() for g in (dx, dy, ds)), tag
            else:
                assert (st[fl] == 12).all() and (its[fl] > 0).all(), (tag, st, its)
                assert np.median(e[fl]) < 1e-6 and e[fl].max() < 5e-3, (tag, e[fl])
        # null tangents: exact zeros
        kw0 = {**kw, "tP_bm": None} if qp else kw
        z = eng.jvp(dv["A_bm"], x, y, s, None, None, **kw0)
        torch.cuda.synchronize()
        for g in z[:3]:
            assert torch.isfinite(g).all() and (g[torch.from_numpy(reg).cuda()] == 0).all(), (tag, "null tangents")
        assert (z[3].cpu().numpy()[reg] == 0).all(), (tag, "null tangents")
        if reg.mean() >= MIN_REGULAR:
            rec["reached"].append((row, _mode_name(kind, "jvp")))

    # ---- the adjoint and the transpose identity (plain kind: k_backward_ns is the adjoint of plain-cone templates alone)
    if kind == "plain":
        from oracle import oracle
        rng = np.random.default_rng(pt["seed"] + 31)
        xb, yb = rng.standard_normal(pt["x"].shape), rng.standard_normal(pt["y"].shape)
        xbt, ybt = torch.from_numpy(xb).cuda(), torch.from_numpy(yb).cuda()
        dA, dq, adj = eng.vjp(dv["A_bm"], x, y, s, xbt, ybt, path="per_instance", lsqr=TIGHT_LSQR, q_eval=dv["q_t"])
        torch.cuda.synchronize()
        adj_n = adj.cpu().numpy()
        g = oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], pt["cones"], pt["x"], pt["y"], pt["s"], xb, yb, mode="dense")
        wantA = _boundary(tpl, g, n)
        eA = _rel(dA.cpu().numpy().T, wantA.T); ec = _rel(dq.cpu().numpy()[:n].T, g["dc"])
        areg = adj_n == 0
        rec.update(adj_share=float(areg.mean()), adj_max=float(max(eA.max(), ec.max())), adj_median=float(np.median(np.maximum(eA, ec))))
        print(f"{tag} adjoint: regular share {areg.mean():.3f} status counts {np.bincount(adj_n).tolist()} dA max {eA.max():.3e} dc max {ec.max():.3e}")
        assert ((adj_n & 3) == 0).all(), (tag, adj_n)
        assert eA.max() < 1e-5 and ec.max() < 1e-5, (tag, eA.max(), ec.max())          # every instance: a flagged one is re-solved under the tight rule
        assert np.abs(dq.cpu().numpy()[n]).max() == 0
        if areg.mean() >= MIN_REGULAR:
            rec["reached"].append((row, _mode_name(kind, "adjoint")))
        if st is not None:
            both = (st == 0) & areg
            lhs = ((xbt * got[0]).sum(dim=1) + (ybt * got[1]).sum(dim=1)).cpu().numpy()
            rhs = ((dA.t() * tA_bm).sum(dim=1) + (dq * tq).sum(dim=0)).cpu().numpy()
            ti = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
            print(f"{tag} transpose identity: max {ti[both].max():.3e}")
            assert (st == adj_n).all(), (tag, st, adj_n)          # the same elimination flags the same instances
            assert (ti[both] < 1e-6).all() and np.abs(lhs[both]).max() > 1e-3, (tag, ti)

    # ---- one Newton step from the planted point moved by 1e-6 relative
    x1, y1, s1, v1 = K.perturbed(pt)
    xt, yt, stt = (torch.from_numpy(a).cuda() for a in (x1, y1, s1))
    xo, yo, so, info = eng.refine(dv["A_bm"], dv["q_t"], xt.clone(), yt.clone(), stt.clone(), 1, status=None, P_bm=dv["P_bm"])
    assert info["path"] == "ns", tag
    torch.cuda.synchronize()
    xo, yo, so = (a.cpu().numpy() for a in (xo, yo, so))
    rst = info["status"].cpu().numpy(); r0, r1 = info["resid_before"].cpu().numpy(), info["resid_after"].cpu().numpy()
    xr, vr, ok = K.dense_newton(pt, x1, v1)
    assert ok.all(), tag
    d_start, d_ref, d_gpu = K.distance(pt, x1, v1), K.distance(pt, xr, vr), K.distance(pt, xo, yo - so)
    kept, flagged = (rst & 1) != 0, (rst & 4) != 0
    rec.update(refine_share=float((kept & ~flagged).mean()), refine_status=np.bincount(rst).tolist(), d_ref=float(d_ref.max()), d_gpu=float(d_gpu.max()))
    print(f"{tag} refine: kept share {(kept & ~flagged).mean():.3f} status counts {np.bincount(rst).tolist()} distance to the planted point: start {d_start.max():.3e}, "
          f"extended-precision dense step {d_ref.max():.3e}, kernel {d_gpu.max():.3e}; rho {r0.max():.3e} -> {r1.max():.3e}")
    assert (r1 <= r0).all(), (tag, r0, r1)
    assert ((rst & 16) == 0).all() and (kept | flagged).all(), (tag, rst)          # a regular planted point 1e-6 away: the step is taken unless the elimination flags
    for a, g in zip((x1, y1, s1), (xo, yo, so)):
        assert np.array_equal(a[flagged], g[flagged]), (tag, "a flagged instance moved")
    sel = kept & ~flagged
    bound = 10 * d_ref + _refine_floor(pt, d_start)
    assert (d_gpu[sel] <= bound[sel]).all(), (tag, d_gpu[sel], d_ref[sel], bound[sel])
    if sel.mean() >= MIN_REGULAR:
        rec["reached"].append((row, _mode_name(kind, "refine")))
    for what in ("jvp", "adj", "refine"):
        share = rec.get(what + "_share")
        if share is not None and share < MIN_REGULAR:
            print(f"{tag}: {what} regular share {share:.3f} below {MIN_REGULAR}: NOT counted as coverage")
    _DONE[name] = rec
    return rec


def _raw_jvp(eng, shape, B=3):
    """ce_jvp / ce_jvp_qp on buffers of a sentinel: (return code, message); asserts that nothing was written"""
    width = max(eng.n, eng.m, eng.nnz_aug, eng.nnz_p if shape[0] == "qp" else 0) + 1
    zf = torch.full((B, width), 7.0, dtype=torch.float64, device="cuda"); zi = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    p, ip, stream = zf.data_ptr(), zi.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if shape[0] == "qp":
        rc = _lib.lib().ce_jvp_qp(eng._h, B, p, eng.nnz_aug, p, p, p, p, p, eng.nnz_aug, None, 0, 0, None, p, p, p, ip, ip, stream)
    else:
        rc = _lib.lib().ce_jvp(eng._h, B, p, eng.nnz_aug, None, 0, 0, p, p, p, p, eng.nnz_aug, None, 0, 0, p, p, p, ip, ip, 1e-8, 1e-8, 1e8, 0, stream)
    msg = _lib.lib().ce_last_error().decode()
    torch.cuda.synchronize()
    assert (zf == 7.0).all() and (zi == 7).all(), (shape, "a refused call wrote")
    return rc, msg


def _raw_refine(eng, shape, B=3):
    width = max(eng.n, eng.m, eng.nnz_aug, eng.nnz_p if shape[0] == "qp" else 0) + 1
    zf = torch.full((B, width), 7.0, dtype=torch.float64, device="cuda"); zi = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    q0 = torch.zeros((eng.n + 1, B), dtype=torch.float64, device="cuda")
    p, ip, stream = zf.data_ptr(), zi.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (eng._h, B, p, eng.nnz_aug, q0.data_ptr(), q0.stride(0), q0.stride(1))
    tail = (p, p, p, None, 1, ip, ip, p, stream)
    rc = _lib.lib().ce_refine_qp(*head, p, *tail) if shape[0] == "qp" else _lib.lib().ce_refine(*head, *tail)
    msg = _lib.lib().ce_last_error().decode()
    torch.cuda.synchronize()
    assert (zf == 7.0).all() and (zi == 7).all(), (shape, "a refused call wrote")
    return rc, msg


def refused_case(name, shape):
    """the first shape past an edge: what include/cone_engine.h documents of a template without the elimination, and no launch of it (nothing is written)"""
    kind, n = shape[0], shape[1]
    tag = f"{name} ({kind}, n {n}, m {P.cone_rows(shape[2])})"
    try:
        tpl, eng = _engine(shape)
    except (NotImplementedError, _lib.EngineError):
        assert pk.host_ns_plan(shape) is None, tag          # ce_create itself refuses the template: the host plan must, too
        print(f"{tag}: refused by ce_create")
        return
    host = _assert_plans_agree(name, shape, eng)
    assert host[pk.NS_KIND_FIELD[kind]] == -1, (tag, host)
    rc, msg = _raw_jvp(eng, shape)
    assert rc == -2, (tag, rc, msg)
    rc, msg = _raw_refine(eng, shape)
    assert rc == -2, (tag, rc, msg)
    pt = K.plant(shape, **K.plant_args(name))
    dv = _device(pt, tpl, shape)
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    t = K.tangents(pt)
    tA_eval, tq_eval = tpl.values_from_dense(*t[:3])
    tA_bm, tq = torch.from_numpy(tA_eval).cuda().t().contiguous(), torch.from_numpy(tq_eval).cuda()
    if kind == "qp":
        with pytest.raises(NotImplementedError):          # (ce_jvp_qp has no LSQR behind it)
            eng.jvp(dv["A_bm"], x, y, s, tA_bm, tq, method="direct", P_bm=dv["P_bm"])
    else:
        try:
            eng.jvp(dv["A_bm"], x, y, s, tA_bm, tq, method="direct", path="per_instance", q_eval=dv["q_t"])
            torch.cuda.synchronize()
            assert eng.last_jvp_kernel == "ce_jvp_lsqr", (tag, eng.last_jvp_kernel)
            print(f"{tag}: ConeEngine.jvp(method='direct') ran ce_jvp_lsqr")
        except NotImplementedError as e:          # the LSQR vectors do not fit either
            print(f"{tag}: ConeEngine.jvp(method='direct') raised: {e}")
    x1, y1, s1, _ = K.perturbed(pt)
    xt, yt, stt = (torch.from_numpy(a).cuda() for a in (x1, y1, s1))
    xo, yo, so, info = eng.refine(dv["A_bm"], dv["q_t"], xt.clone(), yt.clone(), stt.clone(), 1, status=None, P_bm=dv["P_bm"])
    torch.cuda.synchronize()
    assert info["path"] == "none" and info["status"] is None, (tag, info)
    assert torch.equal(xo, xt) and torch.equal(yo, yt) and torch.equal(so, stt), tag


def run_group(group):
    cases = K.cases_of(group)
    assert cases, group
    recs = []
    for name, (shape, plan, what) in cases.items():
        if what == "refused":
            refused_case(name, shape)
        else:
            recs.append(served_case(name, shape, resolve_only=(what == "resolve")))
    return recs


GROUPS = list(pk.NS_FAMILIES) + [f"{name}:{kind}" for name, by in K.STRUCTURE.items() for kind in by]


@pytest.mark.parametrize("group", GROUPS)
def test_modes_at_edges_and_structure_shapes(group):
    recs = run_group(group)
    assert recs, group
    if group.split(":")[0] in K.UNION_LARGEST:
        (rec,) = recs
        abc = pk.ns_union_members(rec["n"], rec["m"], len(K.STRUCTURE[group.split(":")[0]][rec["kind"]][2]["q"]), rec["row"])
        assert abc[K.UNION_LARGEST[group.split(":")[0]]] == max(abc), (group, abc)


def test_refine_through_the_layer_warns_once_past_the_edge():
    """the plugin's side of a refused shape (test_gpu_refine.py::test_templates_without_the_elimination_keep_their_point_and_say_so_once): refine_steps on the first n
    past the column rule returns the solver's point and says so once"""
    from cvxpylayers_amd.interfaces import mi355_if
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    (edge,) = [e for e in K.edge_table() if e[0] == "plain_n" and e[5] is None]
    shape = pk.NS_FAMILIES["plain_n"][2](edge[4])
    pt = K.plant(shape, B=2)
    tpl = P.dense_template(shape[1], shape[2])
    A_eval, q_eval = tpl.values_from_dense(pt["A"], pt["b"], pt["c"])
    ctx = MI355_ctx(None, tpl.problem_data_index, shape[2], options={"eps": 1e-4, "raise_on_error": False})
    A_t, q_t = torch.from_numpy(A_eval).cuda(), torch.from_numpy(q_eval).cuda()
    mi355_if._WARNED.clear()
    with warnings.catch_warnings(record=True) as recw:
        warnings.simplefilter("always")
        p0, d0, info0, _ = _CvxpyLayer.apply(None, q_t, A_t, ctx, {}, True, None)
        p1, d1, info1, _ = _CvxpyLayer.apply(None, q_t, A_t, ctx, {"refine_steps": 1}, True, None)
        p2, d2, info2, _ = _CvxpyLayer.apply(None, q_t, A_t, ctx, {"refine_steps": 1}, True, None)
    torch.cuda.synchronize()
    assert "refine" not in info0 and info1["refine"]["path"] == "none" and info2["refine"]["path"] == "none"
    same = lambda a, b: torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))          # noqa: E731  (a failed instance is masked with NaN on every call)
    assert same(p0, p1) and same(d0, d1) and same(p0, p2)
    said = [w for w in recw if "refine_steps" in str(w.message)]
    assert len(said) == 1, [str(w.message) for w in recw]


def test_ledger_of_rows_and_modes():
    """one entry per (row of CE_NS_VARIANTS, mode of the three NS_MODES lists), both parsed from the sources: a new row or a new mode fails here until a compared
    call at a shape with >= 80 % regular instances reaches it"""
    entries = ledger_entries()
    assert len(entries) == len(pk.variant_rows("CE_NS_VARIANTS")) * len(ns_modes()) and len(set(ns_modes().values())) == len(ns_modes())
    for group in GROUPS:
        if not all(name in _DONE for name, c in K.cases_of(group).items() if c[2] != "refused"):
            run_group(group)
    reached = {}
    for rec in _DONE.values():
        for e in rec["reached"]:
            reached.setdefault(e, []).append(rec)
    print("\nledger (row, mode): shape, regular share, maximum and median error, distance of the extended-precision step and of the kernel's")
    missing = []
    for e in entries:
        if e not in reached:
            print(f"  row {e[0]} {e[1]:12s} NOT REACHED")
            missing.append(e)
            continue
        kind, call = ns_modes()[e[1]]
        rec = max(reached[e], key=lambda r: r["n"] * r["m"])          # the largest shape that reached it
        key = {"jvp": "jvp", "adjoint": "adj", "refine": "refine"}[call]
        extra = f"d_ref {rec['d_ref']:.2e} d_kernel {rec['d_gpu']:.2e}" if call == "refine" else f"max {rec[key + '_max']:.2e} median {rec[key + '_median']:.2e}"
        print(f"  row {e[0]} {e[1]:12s} {rec['name']:28s} n {rec['n']:3d} m {rec['m']:4d} share {rec[key + '_share']:.3f} {extra}  ({len(reached[e])} shapes)")
    assert not missing, missing

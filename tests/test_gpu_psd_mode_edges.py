"""The eight PSD-bearing modes of the search-free elimination k_backward_ns -- NsJvpPsd, NsRefinePsd, NsVjpManyPsd, NsJvpManyPsd (PSD blocks beside plain cones) and
NsJvpPsdTri, NsRefinePsdTri, NsVjpManyPsdTri, NsJvpManyPsdTri (blocks AND exponential / power triples) -- on both sides of every edge of their two planners and at the
smallest structure shapes (psd_edge_kit: the families, the shapes and the planted KKT points; tests/test_psd_edge_kit.py proves every instance regular, the two dense
references transposes of each other and the comparison below sensitive, without a GPU).  Every instance is SOLVED DIRECTLY: what is compared is the elimination's own
answer, not a re-solve.  One engine and one planted point per case, at the planted point with no solve.  Per served case
  * the library's variant and LDS fields equal the host plan's, and the other kind's fields say -1;
  * the forward derivative (ce_jvp_psd / ce_jvp_psd_tri) against psd_tri_ns_kit.dense_jvp on EVERY instance: status-0 instances (>= 80 %) within 1e-5 maximum / 1e-8
    median relative to 1 + max |reference| with no LSQR iteration; a flagged one carries 4 | 8 and meets the flagged bound of test_gpu_jvp_direct.py;
  * one Newton step (ce_refine_psd / ce_refine_psd_tri) from the planted point moved by 1e-6 relative, under the rule and bound of test_gpu_ns_mode_edges.py with
    psd_tri_ns_kit.dense_newton; bit 16 never set;
  * both many modes at K = 4 (g0, g1, 0, g0) against the dense adjoint and the dense forward solve, the same bounds; flags equal across k and equal to the single
    call's; exact zeros for the zero right-hand side; the repeat bit-identical; the K x K transpose identity between the two within 1e-6 (1 + |lhs| + |rhs|).
On the far side of every refusal edge: the kind's variant queries say -1 (LDS 0), the four C entries return CE_E_UNSUPPORTED and write nothing, and ConeEngine.jvp /
refine / jvp_many / vjp_many with the flag take the routes they take without it.
Ledger: the PSD-bearing Ns... structs are parsed from csrc/ce_types.h, the rows from ce_variants.h; every (row, mode) must be reached by a compared call at a shape
with >= 80 % status-0 instances, and a PSD-bearing mode this file does not know fails it."""
import os
import re

import numpy as np
import pytest
import torch

import plan_kit as pk
import psd_edge_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_ns_mode_edges import _boundary

pytestmark = pytest.mark.gpu

_DONE: dict = {}          # case name -> record
EPS = np.finfo(np.float64).eps
KC, ZERO_AT, REPEAT_AT = K.KC, K.ZERO_AT, K.REPEAT_AT
MODES = {"psd": {"jvp": "NsJvpPsd", "refine": "NsRefinePsd", "vjp_many": "NsVjpManyPsd", "jvp_many": "NsJvpManyPsd"},
         "mixed": {"jvp": "NsJvpPsdTri", "refine": "NsRefinePsdTri", "vjp_many": "NsVjpManyPsdTri", "jvp_many": "NsJvpManyPsdTri"}}
ENTRY = {"psd": {"jvp": "ce_jvp_psd", "refine": "ce_refine_psd", "vjp_many": "ce_vjp_psd_many", "jvp_many": "ce_jvp_psd_many"},
         "mixed": {"jvp": "ce_jvp_psd_tri", "refine": "ce_refine_psd_tri", "vjp_many": "ce_vjp_psd_tri_many", "jvp_many": "ce_jvp_psd_tri_many"}}


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for e in pk.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)


def psd_modes():
    """the PSD-bearing mode structs of csrc/ce_types.h"""
    src = open(os.path.join(pk.ROOT, "cvxpylayers_amd", "csrc", "ce_types.h")).read()
    return [nm for nm in re.findall(r"struct (Ns\w+) : \w+ \{\};", src) if "Psd" in nm]


def _engine(shape):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    tpl = P.dense_template(shape[1], shape[2])
    return tpl, ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))


def library_plan(eng):
    L = _lib.lib()
    return {"psd": dict(variant=L.ce_psd_ns_variant(eng._h), lds=L.ce_psd_ns_lds(eng._h), vjp_many=L.ce_vjp_psd_many_variant(eng._h), jvp_many=L.ce_jvp_psd_many_variant(eng._h)),
            "mixed": dict(variant=L.ce_psd_tri_ns_variant(eng._h), lds=L.ce_psd_tri_ns_lds(eng._h), vjp_many=L.ce_vjp_psd_tri_many_variant(eng._h),
                          jvp_many=L.ce_jvp_psd_tri_many_variant(eng._h))}


def assert_plans_agree(tag, shape, eng):
    """the library's fields of both PSD-bearing planners against the host plan; the host plan's row of the shape's kind"""
    host = K.host_plan(shape)
    assert host is not None, tag
    got = library_plan(eng)
    row = host["variant"]
    other = "mixed" if shape[0] == "psd" else "psd"
    assert got[shape[0]] == dict(variant=row, lds=host["lds"], vjp_many=row, jvp_many=row), (tag, got, host)
    assert got[other] == dict(variant=-1, lds=0, vjp_many=-1, jvp_many=-1), (tag, got)
    plan = eng.plan()
    assert plan["ns_variant"] == -1 and plan["tri_ns_variant"] == -1, (tag, plan)
    return row


def _device(pt, tpl):
    A_eval, q_eval = tpl.values_from_dense(pt["A"], pt["b"], pt["c"])
    return dict(A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(), q_t=torch.from_numpy(q_eval).cuda())


def many_tangents(pt, tpl):
    """(KC, B, nnz_aug), (KC, B, n + 1): the draws psd_edge_kit.tangents(pt, 1) and (pt, 2), the zero one, the first again"""
    rows = [tuple(a.T for a in tpl.values_from_dense(*K.tangents(pt, d + 1))) for d in (0, 1)]
    out = []
    for i in range(2):
        a = np.zeros((KC,) + rows[0][i].shape)
        a[0], a[1], a[REPEAT_AT] = rows[0][i], rows[1][i], rows[0][i]
        out.append(a)
    return out


def _refine_floor(pt, d_start):
    """test_gpu_ns_mode_edges._refine_floor with this kit's condition numbers: eps cond(J) |step| and four roundings of the stored point; nothing measured on the kernel"""
    scale = 1 + np.maximum(np.abs(pt["x"]).max(axis=1), np.abs(pt["v"]).max(axis=1))
    return EPS * K.regularity(pt)[0] * d_start + 4 * EPS * scale


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def served_case(name):
    if name in _DONE:
        return _DONE[name]
    shape = K.all_cases()[name][0]
    kind, n = shape[0], shape[1]
    pt = K.case_point(name)
    cond, resid = K.regularity(pt)
    assert (cond <= 1e11).all() and (resid <= 1e-13).all(), (name, cond, resid)
    tpl, eng = _engine(shape)
    row = assert_plans_agree(name, shape, eng)
    assert row >= 0 and row == K.all_cases()[name][1], (name, row)
    dv = _device(pt, tpl)
    B, m = pt["x"].shape[0], pt["m"]
    ent = ENTRY[kind]
    tag = f"{name} ({kind}, n {n}, m {m}, B {B}, row {row})"
    rec = dict(name=name, kind=kind, n=n, m=m, B=B, row=row, reached=[])
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    tA, tq = many_tangents(pt, tpl)
    xb, yb = K.cotangents(pt)
    tAt, tqt, xbt, ybt = (torch.from_numpy(a).cuda() for a in (tA, tq, xb, yb))
    x1, y1, s1, v1 = K.perturbed(pt)
    kw = dict(path="per_instance", lsqr=TIGHT_LSQR, q_eval=dv["q_t"])

    # ---- every launch first, one synchronize
    j1 = eng.jvp(dv["A_bm"], x, y, s, tAt[0], tqt[0].t().contiguous(), method="direct", psd_ns=True, **kw)
    assert eng.last_jvp_kernel == ent["jvp"], (tag, eng.last_jvp_kernel)
    its1 = eng.last_lsqr_iters
    rf = eng.refine(dv["A_bm"], dv["q_t"], *(torch.from_numpy(a).cuda() for a in (x1, y1, s1)), 1, status=None, psd_ns=True)
    assert rf[3]["path"] == "ns", tag
    jm = eng.jvp_many(dv["A_bm"], x, y, s, tAt, tqt, method="direct", psd_many=True, **kw)
    assert (eng.last_jvp_many_path, eng.last_jvp_kernel) == ("many", ent["jvp_many"]), (tag, eng.last_jvp_many_path, eng.last_jvp_kernel)
    itsm = eng.last_lsqr_iters
    vm = eng.vjp_many(dv["A_bm"], x, y, s, xbt, ybt, psd_many=True, **kw)
    assert (eng.last_vjp_many_path, eng.last_vjp_kernel) == ("many", ent["vjp_many"]), (tag, eng.last_vjp_many_path, eng.last_vjp_kernel)
    torch.cuda.synchronize()
    dx1, dy1, ds1, st1, its1 = _np(*j1, its1)
    dx, dy, ds, st, its = _np(*jm, itsm)
    dA, dq, adj = _np(*vm)
    med = K.median_bound(pt)

    # ---- the forward derivative against the dense solve, on every instance
    want = [K.want_forward(pt, d) for d in (0, 1)]
    reg = st1 == 0
    assert ((st1 == 0) | (st1 == 12)).all() and (its1[reg] == 0).all() and (its1[~reg] > 0).all(), (tag, st1, its1)
    w, md = K.hold(tag, ent["jvp"] + " dx, dy, ds", (dx1, dy1, ds1), want[0], reg, med)
    print(f"{tag} {ent['jvp']}: status-0 share {reg.mean():.3f} status counts {np.bincount(st1).tolist()} max {w:.3e} median {md:.3e}")
    assert reg.mean() >= K.MIN_REGULAR, f"{tag}: {ent['jvp']}: status-0 share {reg.mean():.3f} below {K.MIN_REGULAR} -- the reference leaves nothing out"
    rec.update(jvp_share=float(reg.mean()), jvp_max=w, jvp_median=md)

    # ---- one Newton step from the planted point moved by 1e-6 relative (test_gpu_ns_mode_edges.py's rule and bound)
    xo, yo, so = _np(*rf[:3])
    info = rf[3]
    rst, r0, r1 = _np(info["status"], info["resid_before"], info["resid_after"])
    xr, vr, ok = K.dense_newton(pt, x1, v1)
    assert ok.all(), tag
    d_start, d_ref, d_gpu = K.distance(pt, x1, v1), K.distance(pt, xr, vr), K.distance(pt, xo, yo - so)
    kept, flagged = (rst & 1) != 0, (rst & 4) != 0
    sel = kept & ~flagged
    print(f"{tag} {ent['refine']}: kept share {sel.mean():.3f} status counts {np.bincount(rst).tolist()} distance to the planted point: start {d_start.max():.3e}, "
          f"dense step {d_ref.max():.3e}, kernel {d_gpu.max():.3e}; rho {r0.max():.3e} -> {r1.max():.3e}")
    assert (r1 <= r0).all(), (tag, r0, r1)
    assert ((rst & 16) == 0).all() and (kept | flagged).all(), (tag, rst)
    for a, g in zip((x1, y1, s1), (xo, yo, so)):
        assert np.array_equal(a[flagged], g[flagged]), (tag, "a flagged instance moved")
    bound = 10 * d_ref + _refine_floor(pt, d_start)
    assert (d_gpu[sel] <= bound[sel]).all(), (tag, d_gpu[sel], d_ref[sel], bound[sel])
    assert sel.mean() >= K.MIN_REGULAR, f"{tag}: {ent['refine']}: kept share {sel.mean():.3f} below {K.MIN_REGULAR}"
    rec.update(refine_share=float(sel.mean()), d_ref=float(d_ref.max()), d_gpu=float(d_gpu.max()))

    # ---- the many modes: flags are the matrix's
    for what, f in ((ent["jvp_many"], st), (ent["vjp_many"], adj)):
        assert ((f == 0) | (f == 12)).all() and (f == f[:1]).all(), (tag, what, f)
        assert (f[0] == st1).all(), (tag, what, "the single call flags other instances", f[0], st1)
    assert (its[:, reg] == 0).all() and (its[:, ~reg] > 0).all(), (tag, its)

    # ---- against the dense forward solve and the dense adjoint
    worst = np.array([np.nan, np.nan])
    for k, d in K.REF_OF.items():
        worst = np.fmax(worst, K.hold(tag, f"{ent['jvp_many']} k={k} dx, dy, ds", (dx[k], dy[k], ds[k]), want[d], reg, med))
    print(f"{tag} {ent['jvp_many']}: max {worst[0]:.3e} median (largest over k) {worst[1]:.3e}")
    rec.update(jvp_many_share=float(reg.mean()), jvp_many_max=worst[0], jvp_many_median=worst[1])
    g = [K.want_adjoint(pt, d) for d in (0, 1)]
    wantA = [_boundary(tpl, gd, n).T for gd in g]
    worst = np.array([np.nan, np.nan])
    for k, d in K.REF_OF.items():
        worst = np.fmax(worst, K.hold(tag, f"{ent['vjp_many']} k={k} dA, dc", (dA[k], dq[k][:, :n]), (wantA[d], g[d]["dc"]), reg, med))
    print(f"{tag} {ent['vjp_many']}: max {worst[0]:.3e} median (largest over k) {worst[1]:.3e}")
    rec.update(vjp_many_share=float(reg.mean()), vjp_many_max=worst[0], vjp_many_median=worst[1])
    assert (dq[:, :, n] == 0).all(), tag

    # ---- the zero right-hand side, the repeat, the single call
    for what, arrs in ((ent["jvp_many"], (dx, dy, ds)), (ent["vjp_many"], (dA, dq))):
        for a in arrs:
            assert np.isfinite(a).all(), (tag, what)
            assert (a[ZERO_AT][reg] == 0).all(), f"{tag}: {what} k={ZERO_AT}: the zero right-hand side returns {np.abs(a[ZERO_AT][reg]).max():.3e}"
            assert np.array_equal(a[0], a[REPEAT_AT]), f"{tag}: {what} k={REPEAT_AT}: the repeat differs from k=0 by {np.abs(a[0] - a[REPEAT_AT]).max():.3e}"
    for a, b, what in zip((dx, dy, ds), (dx1, dy1, ds1), ("dx", "dy", "ds")):
        e = K.rel(a[0], b)[reg]
        assert e.size == 0 or e.max() < 1e-6, f"{tag}: {ent['jvp_many']} {what} k=0: {e.max():.3e} from the single call"

    # ---- K x K: <xb_k, dx_j> + <yb_k, dy_j> = <dA_k, tA_j> + <dq_k, tq_j>
    lhs = np.einsum("kbi,jbi->kjb", xb, dx) + np.einsum("kbi,jbi->kjb", yb, dy)
    rhs = np.einsum("kbi,jbi->kjb", dA, tA) + np.einsum("kbi,jbi->kjb", dq, tq)
    e = (np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs)))[:, :, reg]
    print(f"{tag} transpose identity: max {e.max():.3e} on {int(reg.sum())} instances, max |lhs| {np.abs(lhs[:, :, reg]).max():.3e}")
    assert e.max() < 1e-6, f"{tag}: transpose identity: {e.max():.3e} above 1e-6"
    assert np.abs(lhs[:, :, reg]).max() > 1e-3, (tag, "the identity is vacuous")

    rec["reached"] = [(row, mode) for mode in MODES[kind].values()]          # (every share was asserted >= MIN_REGULAR above)
    _DONE[name] = rec
    return rec


def _raw_refusals(tag, kind, eng, dv, pt, Kc=2):
    """the kind's four entry points on outputs filled with a sentinel: CE_E_UNSUPPORTED, the entry point named, nothing written"""
    L = _lib.lib()
    B, n, m = pt["x"].shape[0], eng.n, eng.m
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    A_c, q_t = dv["A_bm"].contiguous(), dv["q_t"]
    rng = np.random.default_rng(pt["seed"] + 31)
    xb, yb = torch.from_numpy(rng.standard_normal((Kc, B, n))).cuda(), torch.from_numpy(rng.standard_normal((Kc, B, m))).cuda()
    tA, tq = torch.ones((Kc, B, eng.nnz_aug), **f64), torch.ones((Kc, B, n + 1), **f64)
    o = {k: torch.full((Kc, B) + w, 7.0, **f64) for k, w in dict(dA=(eng.nnz_aug,), dq=(n + 1,), dx=(n,), dy=(m,), ds=(m,)).items()}
    st, its, rst, taken = (torch.full((Kc, B), 7, **i32) for _ in range(4))
    resid = torch.full((B, 2), 7.0, **f64)
    xs, ys, ss = x.clone(), y.clone(), s.clone()
    p = lambda t: t.data_ptr()          # noqa: E731
    qa = (p(q_t), q_t.stride(0), q_t.stride(1))
    fn = {k: getattr(L, v) for k, v in ENTRY[kind].items()}
    calls = {
        "jvp": lambda: fn["jvp"](eng._h, B, p(A_c), eng.nnz_aug, *qa, p(x), p(y), p(s), p(tA), eng.nnz_aug, None, 0, 0, p(o["dx"]), p(o["dy"]), p(o["ds"]), p(st), p(its),
                                 1e-8, 1e-8, 1e8, 0, None),
        "refine": lambda: fn["refine"](eng._h, B, p(A_c), eng.nnz_aug, *qa, p(xs), p(ys), p(ss), None, 1, p(rst), p(taken), p(resid), None),
        "vjp_many": lambda: fn["vjp_many"](eng._h, B, Kc, p(A_c), eng.nnz_aug, *qa, p(x), p(y), p(s), p(xb), p(yb), p(o["dA"]), p(o["dq"]), p(st), None),
        "jvp_many": lambda: fn["jvp_many"](eng._h, B, Kc, p(A_c), eng.nnz_aug, *qa, p(x), p(y), p(s), p(tA), tA.stride(0), eng.nnz_aug, p(tq), tq.stride(0), n + 1,
                                           p(o["dx"]), p(o["dy"]), p(o["ds"]), p(st), p(its), 1e-8, 1e-8, 1e8, 0, None),
    }
    for who, call in calls.items():
        rc = call()
        msg = (L.ce_last_error() or b"").decode()
        assert rc == -2 and ENTRY[kind][who] + ":" in msg, (tag, who, rc, msg)
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in o.values()) and all((t == 7).all() for t in (st, its, rst, taken)) and (resid == 7.0).all(), (tag, "a refused call wrote")
    assert torch.equal(xs, x) and torch.equal(ys, y) and torch.equal(ss, s), (tag, "a refused ce_refine moved the point")
    return xb, yb, tA, tq


def _as_the_single_calls(tag, what, many, single, Kc):
    """many() is torch.equal to the stacked single(k), or raises what single raises (test_gpu_ns_many_edges.py)"""
    try:
        ones = [single(k) for k in range(Kc)]
    except (NotImplementedError, _lib.EngineError, ValueError) as exc:
        with pytest.raises(type(exc)):
            many()
        print(f"{tag}: {what} and its single call both raise {type(exc).__name__}")
        return
    got = many()
    torch.cuda.synchronize()
    for i, g in enumerate(got):
        assert torch.equal(g, torch.stack([o[i] for o in ones])), (tag, what, i)
    print(f"{tag}: {what} ran the loop and equals {Kc} single calls")


def refused_case(name):
    """the first shape past a refusal edge: -1 from every query, no launch (nothing is written), and the routes of a call without the flag"""
    shape, row, gate = K.all_cases()[name]
    kind, n = shape[0], shape[1]
    tag = f"{name} ({kind}, n {n}, m {P.cone_rows(shape[2])}, gate {gate})"
    assert row == -1 and gate in K.GATES, tag
    tpl, eng = _engine(shape)
    got = library_plan(eng)
    assert got["psd"] == got["mixed"] == dict(variant=-1, lds=0, vjp_many=-1, jvp_many=-1), (tag, got)
    assert eng.psd_ns_variant == -1 and eng.psd_tri_ns_variant == -1, tag
    Kc = 2
    pt = K.plant(shape, B=2, **K.plant_args(name))
    dv = _device(pt, tpl)
    xb, yb, tA, tq = _raw_refusals(tag, kind, eng, dv, pt, Kc)
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    A_bm = dv["A_bm"]
    kw = dict(path="per_instance", lsqr=TIGHT_LSQR, q_eval=dv["q_t"])
    try:
        eng.jvp(A_bm, x, y, s, tA[0], tq[0].t().contiguous(), method="direct", psd_ns=True, **kw)
        torch.cuda.synchronize()
        assert eng.last_jvp_kernel == "ce_jvp_lsqr", (tag, eng.last_jvp_kernel)
        print(f"{tag}: ConeEngine.jvp(method='direct', psd_ns=True) ran ce_jvp_lsqr")
    except NotImplementedError as e:          # the LSQR vectors do not fit either
        assert gate == "resolve", (tag, e)
        print(f"{tag}: ConeEngine.jvp(method='direct', psd_ns=True) raised: {e}")
    _as_the_single_calls(tag, "vjp_many(psd_many=True)", lambda: eng.vjp_many(A_bm, x, y, s, xb, yb, psd_many=True, **kw),
                         lambda k: (lambda o: (o[0].t(), o[1].t(), o[2]))(eng.vjp(A_bm, x, y, s, xb[k], yb[k], **kw)), Kc)
    assert eng.last_vjp_many_path == "loop", tag
    _as_the_single_calls(tag, "jvp_many(psd_many=True)", lambda: eng.jvp_many(A_bm, x, y, s, tA, tq, method="direct", psd_many=True, **kw),
                         lambda k: eng.jvp(A_bm, x, y, s, tA[k], tq[k].t().contiguous(), method="direct", **kw), Kc)
    assert eng.last_jvp_many_path == "loop", tag
    x1, y1, s1, _ = K.perturbed(pt)
    xt, yt, stt = (torch.from_numpy(a).cuda() for a in (x1, y1, s1))
    xo, yo, so, info = eng.refine(A_bm, dv["q_t"], xt.clone(), yt.clone(), stt.clone(), 1, status=None, psd_ns=True)
    torch.cuda.synchronize()
    assert info["path"] == "none" and info["status"] is None, (tag, info)
    assert torch.equal(xo, xt) and torch.equal(yo, yt) and torch.equal(so, stt), tag


def run_group(group):
    cases = K.cases_of(group)
    assert cases, group
    recs = []
    for name, (shape, row, gate) in cases.items():
        if row >= 0:
            recs.append(served_case(name))
        else:
            refused_case(name)
    return recs


@pytest.mark.parametrize("group", K.GROUPS)
def test_psd_modes_at_edges_and_structure_shapes(group):
    recs = run_group(group)
    assert recs, group
    if group.split(":")[0] in K.STRUCTURE_ROW:
        assert recs[0]["row"] == K.STRUCTURE_ROW[group.split(":")[0]], (group, recs[0]["row"])


def test_ledger_of_rows_and_psd_modes():
    """one entry per (row of CE_NS_VARIANTS, PSD-bearing mode of csrc/ce_types.h): a new row or a new PSD-bearing mode fails here until a compared call at a shape with
    >= 80 % status-0 instances reaches it; the near side of a refusal by each gate of the plan must have been compared on row 0"""
    mine = [mode for by in MODES.values() for mode in by.values()]
    assert sorted(psd_modes()) == sorted(mine), (psd_modes(), "a PSD-bearing mode without an edge ledger")
    rows = [r[0] for r in pk.variant_rows("CE_NS_VARIANTS")]
    for group in K.GROUPS:
        if not all(name in _DONE for name, c in K.cases_of(group).items() if c[1] >= 0):
            run_group(group)
    reached = {}
    for rec in _DONE.values():
        for e in rec["reached"]:
            reached.setdefault(e, []).append(rec)
    print("\nledger (row, mode, entry point): shapes that reached it; over them: worst and largest median error against the dense reference (refine: largest distance to "
          "the planted point of the dense step and of the kernel's)")
    missing = []
    for kind, by in MODES.items():
        for row in rows:
            for call, mode in by.items():
                recs = reached.get((row, mode), [])
                if not recs:
                    print(f"  row {row} {mode:16s} {ENTRY[kind][call]:20s} NOT REACHED"); missing.append((row, mode))
                    continue
                fig = (f"d_ref {max(r['d_ref'] for r in recs):.2e} d_kernel {max(r['d_gpu'] for r in recs):.2e}" if call == "refine" else
                       f"max {np.nanmax([r[call + '_max'] for r in recs]):.2e} median {np.nanmax([r[call + '_median'] for r in recs]):.2e}")
                print(f"  row {row} {mode:16s} {ENTRY[kind][call]:20s} {len(recs):2d} shapes, smallest share {min(r[call + '_share'] for r in recs):.3f}, {fig}")
    assert not missing, missing
    assert len(rows) * len(mine) == 24 == len({e for e in reached if e[1] in mine}), (rows, mine)
    for gate in ("footprint", "resolve"):
        near = [f"{fam}:{kind}[{vb}]" for fam, kind, vb, rb, va, ra, g in K.edge_table() if g == gate]
        assert near and all(nm in _DONE and _DONE[nm]["row"] == 0 for nm in near), (gate, near)
        print(f"  near side of a refusal by the {gate} gate, compared on row 0: {near}")

"""The four many-right-hand-side modes of the search-free elimination that are objects of their own beside csrc/ce_tu_ns.hip -- NsMany (ce_vjp_many), NsJvpMany
(ce_jvp_many), NsJvpQpMany (ce_jvp_qp_many), NsVjpQpMany (ce_vjp_qp_many) -- at the edges of the plain and the QP planner and at the structure shapes of
ns_edge_kit: every `plain` and `qp` case of ns_edge_kit.all_cases(), at the kit's planted points and batch sizes (tests/test_ns_edge_kit.py proves every instance
regular and the two references transposes of each other without a GPU).  The fifth such mode, NsVjpTriMany, has tests/test_gpu_vjp_tri_many_edges.py.

Each mode factors an instance once and rebuilds per right-hand side what the prologue, the classification pass and the sweep left in LDS, from retained state the
single-right-hand-side modes never read again.  So K = 4 right-hand sides (g0, g1, 0, g0) at every served shape: a leftover of g0 shows in g1 against its
reference, a leftover of g1 as a non-zero answer to the zero one, and the repeat shows anything that accumulates.  One engine and one planted point per case serve
both modes of its kind.  Per served shape
  * the library's variant of both modes equals the host plan's row (plain kind: -1 where the LSQR vectors of the re-solve do not fit) and the call takes the "many" route;
  * the adjoint against the oracle's dense elimination (QP kind: with P, dP included, a one-triangle entry doubled), the forward derivative against the dense solve
    on every instance: status-0 instances within 1e-5 (forward: and 1e-8 median, no LSQR iteration) relative to 1 + max |reference|; plain kind: flagged ones (4 | 8)
    re-solved under TIGHT_LSQR to the flagged bound (median 1e-6, maximum 5e-3); QP kind: flagged ones keep status 4, no iteration, finite numbers;
  * the flags are the matrix's: equal for every k, equal to those of one single-right-hand-side call at the point, bits 0-1 never set;
  * the zero right-hand side returns exact zeros on status-0 instances; the repeat is bit-identical (ce_vjp_many: within 1e-6, the bound of its own file);
  * the loop of single calls (QP adjoint: the pivoting kernel, on the instances unflagged by both) within 1e-6;
  * the K x K transpose identity between the two modes of the kind where both report status 0.
On the first refused shape past each edge: all four entry points return CE_E_UNSUPPORTED with a message that names them and write nothing, the variant accessors
return -1, and ConeEngine.vjp_many / jvp_many at K = 2 do exactly what two single calls do.
Ledger: the Ns...Many overloads of ce_launch_ns are parsed from csrc/ce_types.h; every (row of CE_NS_VARIANTS, mode) of the four must be reached by a compared
call at a shape where >= 80 % of the instances have status 0."""
import os
import re

import numpy as np
import pytest
import torch

import ns_edge_kit as K
import plan_kit as pk
from cvxpylayers_amd import _lib
from kit import TIGHT_LSQR
from test_gpu_ns_mode_edges import MIN_REGULAR, _assert_plans_agree, _boundary, _device, _engine, _rel
from test_gpu_vjp_qp_many import _dp_values
from test_quad_objective import _p_values

pytestmark = pytest.mark.gpu

_DONE: dict = {}          # case name -> record
KC = 4
REF_OF = {0: 0, 1: 1, 3: 0}          # position -> Gaussian draw (position 2 is the zero right-hand side)
ZERO_AT, REPEAT_AT = 2, 3
MODES = {"plain": {"adjoint": "NsMany", "jvp": "NsJvpMany"}, "qp": {"adjoint": "NsVjpQpMany", "jvp": "NsJvpQpMany"}}
ELSEWHERE = {"NsVjpTriMany": "tests/test_gpu_vjp_tri_many_edges.py"}
ENTRY = {"NsMany": "ce_vjp_many", "NsJvpMany": "ce_jvp_many", "NsJvpQpMany": "ce_jvp_qp_many", "NsVjpQpMany": "ce_vjp_qp_many"}


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for e in pk.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)


def many_modes():
    """the mode structs of the ce_launch_ns(... const Ns...Many &w) overloads of csrc/ce_types.h"""
    src = open(os.path.join(pk.ROOT, "cvxpylayers_amd", "csrc", "ce_types.h")).read()
    return re.findall(r"int ce_launch_ns\([^;]*const (Ns\w*Many) &w\);", src)


def cases_of(group=None):
    every = {k: c for k, c in K.all_cases().items() if c[0][0] in MODES}
    return every if group is None else {k: c for k, c in every.items() if k == group or k.startswith(group + "[")}


GROUPS = [f for f in pk.NS_FAMILIES if pk.NS_FAMILIES[f][0] in MODES] + [f"{name}:{kind}" for name, by in K.STRUCTURE.items() for kind in by if kind in MODES]


def many_variant(kind, host):
    """the row the many modes of the kind run on by the host plan (include/cone_engine.h ce_*_many_variant), -1: refused"""
    if host is None:
        return -1
    return host["qp_ns_variant"] if kind == "qp" else (host["ns_variant"] if host["resolve_fits"] else -1)


def cotangents(pt):
    """(KC, B, n), (KC, B, m): two draws of default_rng(seed + 31) -- the first is the one of test_gpu_ns_mode_edges.py -- the zero one, the first again"""
    rng = np.random.default_rng(pt["seed"] + 31)
    xb = np.zeros((KC,) + pt["x"].shape); yb = np.zeros((KC,) + pt["y"].shape)
    for k in (0, 1):
        xb[k] = rng.standard_normal(pt["x"].shape); yb[k] = rng.standard_normal(pt["y"].shape)
    xb[REPEAT_AT], yb[REPEAT_AT] = xb[0], yb[0]
    return xb, yb


def tangents(pt, tpl, struct):
    """the dense draws ns_edge_kit.tangents(pt, seed=1), (pt, seed=2) and (KC, B, .) value rows tA, tq, tP (QP kind, else None) laid out as the cotangents are"""
    dense = [K.tangents(pt, seed=1), K.tangents(pt, seed=2)]
    rows = []
    for t in dense:
        tA_eval, tq_eval = tpl.values_from_dense(*t[:3])
        rows.append((tA_eval.T, tq_eval.T, None if t[3] is None else _p_values(t[3], struct)))
    out = []
    for i in range(3):
        if rows[0][i] is None:
            out.append(None)
            continue
        a = np.zeros((KC,) + rows[0][i].shape)
        a[0], a[1], a[REPEAT_AT] = rows[0][i], rows[1][i], rows[0][i]
        out.append(a)
    return dense, out


def hold(tag, what, k, e, reg, median=False, flagged_bound=True):
    """the bounds of one compared right-hand side: e the per-instance error relative to 1 + max |reference|, reg the status-0 instances.  Status 0: maximum 1e-5
    (median 1e-8 where the mode's single-right-hand-side twin is held to it); flagged, where a re-solve stands behind the mode: median 1e-6, maximum 5e-3.
    Returns (largest status-0 error, largest flagged error), nan where there is no such instance."""
    if reg.any():
        assert e[reg].max() < 1e-5, f"{tag}: {what} k={k}: status-0 error {e[reg].max():.3e} (instance {int(np.nonzero(reg)[0][e[reg].argmax()])}) above 1e-5"
        if median:
            assert np.median(e[reg]) < 1e-8, f"{tag}: {what} k={k}: status-0 median error {np.median(e[reg]):.3e} above 1e-8"
    if (~reg).any() and flagged_bound:
        assert np.median(e[~reg]) < 1e-6 and e[~reg].max() < 5e-3, f"{tag}: {what} k={k}: flagged errors {e[~reg].tolist()} above median 1e-6 / maximum 5e-3"
    return (float(e[reg].max()) if reg.any() else float("nan")), (float(e[~reg].max()) if (~reg).any() else float("nan"))


def hold_against_the_loop(tag, what, got, loop, sel):
    """(K, B, .) arrays of the many call and of the loop of single calls: within 1e-6 relative to 1 + max |loop| on the instances sel (B,)"""
    e = _rel(got.reshape(-1, got.shape[-1]), loop.reshape(-1, loop.shape[-1])).reshape(got.shape[:2])[:, sel]
    if e.size:
        k, i = np.unravel_index(e.argmax(), e.shape)
        assert e.max() < 1e-6, f"{tag}: {what} k={k}: {e.max():.3e} from the loop of single calls (instance {int(np.nonzero(sel)[0][i])}) above 1e-6"
    return float(e.max()) if e.size else 0.0


def hold_identity(tag, lhs, rhs, both, scale):
    """K x K transpose identity on the instances both modes solve: lhs, rhs (K, K, B)"""
    if not both.any():
        print(f"{tag} transpose identity: no instance with status 0 in both modes")
        return
    e = (np.abs(lhs - rhs) / scale(np.abs(lhs), np.abs(rhs)))[:, :, both]
    k, j, _ = np.unravel_index(e.argmax(), e.shape)
    print(f"{tag} transpose identity: max {e.max():.3e} on {int(both.sum())} instances, max |lhs| {np.abs(lhs[:, :, both]).max():.3e}")
    assert e.max() < 1e-6, f"{tag}: transpose identity cotangent {k} tangent {j}: {e.max():.3e} above 1e-6"
    assert np.abs(lhs[:, :, both]).max() > 1e-3, (tag, "the identity is vacuous")


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def served_case(name, shape):
    if name in _DONE:
        return _DONE[name]
    kind, n = shape[0], shape[1]
    pt = K.point(name, shape, **K.plant_args(name))
    cond, resid = K.regularity(pt)
    assert (cond <= 1e11).all() and (resid <= 1e-13).all(), (name, cond, resid)
    tpl, eng = _engine(shape)
    host = _assert_plans_agree(name, shape, eng)
    row = many_variant(kind, host)
    assert row >= 0, (name, host)
    L = _lib.lib()
    got_rows = dict(vjp_many=L.ce_vjp_many_variant(eng._h), jvp_many=L.ce_jvp_many_variant(eng._h), jvp_qp_many=L.ce_jvp_qp_many_variant(eng._h),
                    vjp_qp_many=L.ce_vjp_qp_many_variant(eng._h))
    want_rows = dict(vjp_many=-1, jvp_many=-1, jvp_qp_many=row, vjp_qp_many=row) if kind == "qp" else dict(vjp_many=row, jvp_many=row, jvp_qp_many=-1, vjp_qp_many=-1)
    assert got_rows == want_rows, (name, got_rows, want_rows)
    dv = _device(pt, tpl, shape)
    B, m = pt["x"].shape[0], pt["m"]
    rec = dict(name=name, kind=kind, n=n, m=m, B=B, row=row, nq=len(shape[2]["q"]), reached=[])
    tag = f"{name} ({kind}, n {n}, m {m}, B {B}, row {row})"
    (qp_case if kind == "qp" else plain_case)(tag, pt, tpl, eng, dv, rec)
    for call, mode in MODES[kind].items():
        share = rec[call + "_share"]
        if share >= MIN_REGULAR:
            rec["reached"].append((row, mode))
        else:
            print(f"{tag}: {ENTRY[mode]} status-0 share {share:.3f} below {MIN_REGULAR}: NOT counted as coverage")
    _DONE[name] = rec
    return rec


def plain_case(tag, pt, tpl, eng, dv, rec):
    from oracle import oracle
    n, B = pt["n"], pt["x"].shape[0]
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    xb, yb = cotangents(pt)
    dense_t, (tA, tq, _) = tangents(pt, tpl, None)
    xbt, ybt, tAt, tqt = (torch.from_numpy(a).cuda() for a in (xb, yb, tA, tq))
    kw = dict(path="per_instance", lsqr=TIGHT_LSQR, q_eval=dv["q_t"])
    # ---- every launch first, one synchronize
    vm = eng.vjp_many(dv["A_bm"], x, y, s, xbt, ybt, **kw)
    assert eng.last_vjp_many_path == "many" and eng.last_vjp_kernel == "ce_vjp_many", (tag, eng.last_vjp_many_path, eng.last_vjp_kernel)
    vl = eng.vjp_many(dv["A_bm"], x, y, s, xbt, ybt, force_loop=True, **kw)
    assert eng.last_vjp_many_path == "loop", tag
    v1 = eng.vjp(dv["A_bm"], x, y, s, xbt[0], ybt[0], **kw)
    jm = eng.jvp_many(dv["A_bm"], x, y, s, tAt, tqt, method="direct", **kw)
    assert eng.last_jvp_many_path == "many" and eng.last_jvp_kernel == "ce_jvp_many", (tag, eng.last_jvp_many_path, eng.last_jvp_kernel)
    its = eng.last_lsqr_iters
    jl = eng.jvp_many(dv["A_bm"], x, y, s, tAt, tqt, method="direct", force_loop=True, **kw)
    assert eng.last_jvp_many_path == "loop", tag
    j1 = eng.jvp(dv["A_bm"], x, y, s, tAt[0], tqt[0].t(), method="direct", **kw)
    assert eng.last_jvp_kernel == "ce_jvp", tag
    torch.cuda.synchronize()
    dA, dq, adj = _np(*vm); dA_l, dq_l, adj_l = _np(*vl); adj_1 = v1[2].cpu().numpy()
    dx, dy, ds, st, its = _np(*jm, its); dx_l, dy_l, ds_l, st_l = _np(*jl); st_1 = j1[3].cpu().numpy()

    # ---- flags: the matrix's
    for what, f, f_l, f_1 in (("ce_vjp_many", adj, adj_l, adj_1), ("ce_jvp_many", st, st_l, st_1)):
        assert ((f & (4 | 8)) == (f[:1] & (4 | 8))).all() and ((f & 3) == 0).all() and ((f == 0) | (f == 12)).all(), (tag, what, f)
        assert (f == f_l).all(), (tag, what, "the loop flags other instances", f, f_l)
        assert (f[0] == f_1).all(), (tag, what, "one single call flags other instances", f[0], f_1)
    assert (adj[0] == st[0]).all(), (tag, "the same elimination flags the same instances", adj[0], st[0])
    reg = adj[0] == 0
    rec.update(adjoint_share=float(reg.mean()), jvp_share=float(reg.mean()))

    # ---- the adjoint against the oracle's dense elimination
    g = [oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], pt["cones"], pt["x"], pt["y"], pt["s"], xb[k], yb[k], mode="dense") for k in (0, 1)]
    wantA = [_boundary(tpl, gk, n).T for gk in g]
    worst = [np.nan, np.nan]
    for k, d in REF_OF.items():
        e = np.maximum(_rel(dA[k], wantA[d]), _rel(dq[k][:, :n], g[d]["dc"]))
        print(f"{tag} ce_vjp_many k={k}: status-0 share {reg.mean():.3f} status counts {np.bincount(adj[k]).tolist()} error max {e.max():.3e}" +
              (f", flagged {e[~reg].tolist()}" if (~reg).any() else ""))
        worst = np.fmax(worst, hold(tag, "ce_vjp_many dA, dc", k, e, reg))
    rec.update(adjoint_max=worst[0], adjoint_flagged=worst[1])
    assert (dq[:, :, n] == 0).all(), tag

    # ---- the forward derivative against the dense solve
    want = [K.dense_jvp(pt, t) for t in dense_t]
    assert all(w[3].all() for w in want), tag          # no instance left out on the reference's account
    worst = [np.nan, np.nan]
    for k, d in REF_OF.items():
        e = np.max([_rel(a[k], w) for a, w in zip((dx, dy, ds), want[d][:3])], axis=0)
        print(f"{tag} ce_jvp_many k={k}: status counts {np.bincount(st[k]).tolist()} error max {e.max():.3e}" + (f" median {np.median(e[reg]):.3e}" if reg.any() else "") +
              (f", flagged: iterations {its[k][~reg].tolist()} error {e[~reg].tolist()}" if (~reg).any() else ""))
        worst = np.fmax(worst, hold(tag, "ce_jvp_many dx, dy, ds", k, e, reg, median=True))
    rec.update(jvp_max=worst[0], jvp_flagged=worst[1])
    assert (its[:, reg] == 0).all() and (its[:, ~reg] > 0).all(), (tag, its)

    # ---- the zero right-hand side, the repeat, the loop
    for what, arrs in (("ce_vjp_many", (dA, dq)), ("ce_jvp_many", (dx, dy, ds))):
        for a in arrs:
            assert np.isfinite(a).all(), (tag, what)
            assert (a[ZERO_AT][reg] == 0).all(), f"{tag}: {what} k={ZERO_AT}: the zero right-hand side returns {np.abs(a[ZERO_AT][reg]).max():.3e}"
    for a, what in zip((dx, dy, ds), ("dx", "dy", "ds")):
        assert np.array_equal(a[0], a[REPEAT_AT]), f"{tag}: ce_jvp_many {what} k={REPEAT_AT}: the repeat differs from k=0 by {np.abs(a[0] - a[REPEAT_AT]).max():.3e}"
    for a, what in zip((dA, dq), ("dA", "dq")):
        e = _rel(a[REPEAT_AT], a[0])
        assert e.max() < 1e-6, f"{tag}: ce_vjp_many {what} k={REPEAT_AT}: the repeat differs from k=0 by {e.max():.3e}"
    every = np.ones(B, bool)
    el = max(hold_against_the_loop(tag, "ce_vjp_many " + w, a, b, every) for w, a, b in (("dA", dA, dA_l), ("dq", dq, dq_l)))
    ej = max(hold_against_the_loop(tag, "ce_jvp_many " + w, a, b, every) for w, a, b in (("dx", dx, dx_l), ("dy", dy, dy_l), ("ds", ds, ds_l)))
    print(f"{tag} against the loops: ce_vjp_many {el:.3e}, ce_jvp_many {ej:.3e}")

    # ---- K x K: <xb_k, dx_j> + <yb_k, dy_j> = <dA_k, tA_j> + <dq_k, tq_j>
    lhs = np.einsum("kbi,jbi->kjb", xb, dx) + np.einsum("kbi,jbi->kjb", yb, dy)
    rhs = np.einsum("kbi,jbi->kjb", dA, tA) + np.einsum("kbi,jbi->kjb", dq, tq)
    hold_identity(tag, lhs, rhs, (adj == 0).all(axis=0) & (st == 0).all(axis=0), lambda a, b: 1 + a + b)


def qp_case(tag, pt, tpl, eng, dv, rec):
    from oracle import oracle
    n, B = pt["n"], pt["x"].shape[0]
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    xb, yb = cotangents(pt)
    dense_t, (tA, tq, tP) = tangents(pt, tpl, dv["struct"])
    xbt, ybt, tAt, tqt, tPt = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (xb, yb, tA, tq, tP))
    # ---- every launch first, one synchronize
    jm = eng.jvp_many(dv["A_bm"], x, y, s, tAt, tqt, method="direct", P_bm=dv["P_bm"], tP=tPt)
    assert eng.last_jvp_many_path == "many" and eng.last_jvp_kernel == "ce_jvp_qp_many", (tag, eng.last_jvp_many_path, eng.last_jvp_kernel)
    its = eng.last_lsqr_iters
    jl = eng.jvp_many(dv["A_bm"], x, y, s, tAt, tqt, method="direct", P_bm=dv["P_bm"], tP=tPt, force_loop=True)
    assert eng.last_jvp_many_path == "loop" and eng.last_jvp_kernel == "ce_jvp_qp", tag
    vm = eng.vjp_many(dv["A_bm"], x, y, s, xbt, ybt, path="per_instance", P_bm=dv["P_bm"], qp_many=True)
    assert eng.last_vjp_many_path == "many" and eng.last_vjp_kernel == "ce_vjp_qp_many", (tag, eng.last_vjp_many_path, eng.last_vjp_kernel)
    vl = eng.vjp_many(dv["A_bm"], x, y, s, xbt, ybt, path="per_instance", P_bm=dv["P_bm"], qp_many=False)          # (the pivoting kernel: another algorithm)
    assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None, tag
    torch.cuda.synchronize()
    dx, dy, ds, st, its = _np(*jm, its); dx_l, dy_l, ds_l, st_l = _np(*jl)
    dA, dq, adj, dP = _np(*vm); dA_l, dq_l, adj_l, dP_l = _np(*vl)

    # ---- flags: status 4 for every k, never 4 | 8, no iteration; the bit-4 set is ce_jvp_qp's (the loop's first call)
    for what, f in (("ce_jvp_qp_many", st), ("ce_vjp_qp_many", adj)):
        assert ((f & ~4) == 0).all() and (f == f[:1]).all(), (tag, what, f)
        assert (f[0] == st_l[0]).all(), (tag, what, "ce_jvp_qp flags other instances", f[0], st_l[0])
    assert (st == st_l).all() and (its == 0).all(), (tag, st, st_l, its)
    reg = st[0] == 0
    rec.update(adjoint_share=float(reg.mean()), jvp_share=float(reg.mean()))

    # ---- the forward derivative against the dense solve (a flagged instance keeps the dropped-variable answer: finite, not compared)
    want = [K.dense_jvp(pt, t) for t in dense_t]
    assert all(w[3].all() for w in want), tag
    worst = [np.nan, np.nan]
    for k, d in REF_OF.items():
        e = np.max([_rel(a[k], w) for a, w in zip((dx, dy, ds), want[d][:3])], axis=0)
        print(f"{tag} ce_jvp_qp_many k={k}: status counts {np.bincount(st[k]).tolist()} error max {e.max():.3e}" + (f" median {np.median(e[reg]):.3e}" if reg.any() else "") +
              (f", flagged {e[~reg].tolist()}" if (~reg).any() else ""))
        worst = np.fmax(worst, hold(tag, "ce_jvp_qp_many dx, dy, ds", k, e, reg, median=True, flagged_bound=False))
    rec.update(jvp_max=worst[0], jvp_flagged=worst[1])

    # ---- the adjoint against the oracle's dense elimination with P: dA, dq and dP
    g = [oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], pt["cones"], pt["x"], pt["y"], pt["s"], xb[k], yb[k], P=pt["Pm"], mode="dense") for k in (0, 1)]
    wantA = [_boundary(tpl, gk, n).T for gk in g]
    wantP = [_dp_values(gk["dP"], dv["struct"]) for gk in g]
    worst = [np.nan, np.nan]
    for k, d in REF_OF.items():
        e = np.max([_rel(dA[k], wantA[d]), _rel(dq[k][:, :n], g[d]["dc"]), _rel(dP[k], wantP[d])], axis=0)
        print(f"{tag} ce_vjp_qp_many k={k}: status counts {np.bincount(adj[k]).tolist()} error max {e.max():.3e}" + (f", flagged {e[~reg].tolist()}" if (~reg).any() else ""))
        worst = np.fmax(worst, hold(tag, "ce_vjp_qp_many dA, dq, dP", k, e, reg, flagged_bound=False))
    rec.update(adjoint_max=worst[0], adjoint_flagged=worst[1])
    assert (dq[:, :, n] == 0).all(), tag

    # ---- the zero right-hand side, the repeat, the loops
    for what, arrs in (("ce_jvp_qp_many", (dx, dy, ds)), ("ce_vjp_qp_many", (dA, dq, dP))):
        for a in arrs:
            assert np.isfinite(a).all(), (tag, what)
            assert (a[ZERO_AT][reg] == 0).all(), f"{tag}: {what} k={ZERO_AT}: the zero right-hand side returns {np.abs(a[ZERO_AT][reg]).max():.3e}"
            assert np.array_equal(a[0], a[REPEAT_AT]), f"{tag}: {what} k={REPEAT_AT}: the repeat differs from k=0 by {np.abs(a[0] - a[REPEAT_AT]).max():.3e}"
    sel = reg & (st_l == 0).all(axis=0)
    ej = max(hold_against_the_loop(tag, "ce_jvp_qp_many " + w, a, b, sel) for w, a, b in (("dx", dx, dx_l), ("dy", dy, dy_l), ("ds", ds, ds_l)))
    sel = reg & (adj_l == 0).all(axis=0)
    el = max(hold_against_the_loop(tag, "ce_vjp_qp_many " + w, a, b, sel) for w, a, b in (("dA", dA, dA_l), ("dq", dq, dq_l), ("dP", dP, dP_l)))
    print(f"{tag} against the loops: ce_jvp_qp_many {ej:.3e}, ce_vjp_qp_many {el:.3e} (pivoting kernel; it flags {int((adj_l[0] != 0).sum())})")

    # ---- K x K with the P block, in the boundary's coordinates (test_gpu_vjp_qp_many.py)
    lhs = np.einsum("kbi,jbi->kjb", xb, dx) + np.einsum("kbi,jbi->kjb", yb, dy)
    rhs = np.einsum("kbi,jbi->kjb", dA, tA) + np.einsum("kbi,jbi->kjb", dq, tq) + np.einsum("kbi,jbi->kjb", dP, tP)
    hold_identity(tag, lhs, rhs, reg, lambda a, b: 1 + np.maximum(a, b))


def _raw_refusals(tag, eng, dv, pt, Kc):
    """all four entry points on outputs filled with a sentinel: CE_E_UNSUPPORTED, the entry point named, nothing written"""
    L = _lib.lib()
    B, n, m = pt["x"].shape[0], eng.n, eng.m
    f64 = dict(dtype=torch.float64, device="cuda")
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    A_c, q_t = dv["A_bm"].contiguous(), dv["q_t"]
    nnzp = max(eng.nnz_p, 1)
    P_c = dv["P_bm"].contiguous() if dv["P_bm"] is not None else torch.zeros((B, nnzp), **f64)
    rng = np.random.default_rng(pt["seed"] + 31)
    xb, yb = torch.from_numpy(rng.standard_normal((Kc, B, n))).cuda(), torch.from_numpy(rng.standard_normal((Kc, B, m))).cuda()
    tA, tq, tP = torch.ones((Kc, B, eng.nnz_aug), **f64), torch.ones((Kc, B, n + 1), **f64), torch.ones((Kc, B, nnzp), **f64)
    outs = dict(dA=(eng.nnz_aug,), dq=(n + 1,), dP=(nnzp,), dx=(n,), dy=(m,), ds=(m,))
    o = {k: torch.full((Kc, B) + w, 7.0, **f64) for k, w in outs.items()}
    st, its = (torch.full((Kc, B), 7, dtype=torch.int32, device="cuda") for _ in range(2))
    p = lambda t: t.data_ptr()          # noqa: E731
    point = (p(x), p(y), p(s))
    tang = (p(tA), tA.stride(0), eng.nnz_aug, p(tq), tq.stride(0), n + 1)
    calls = {
        "ce_vjp_many": lambda: L.ce_vjp_many(eng._h, B, Kc, p(A_c), eng.nnz_aug, p(q_t), q_t.stride(0), q_t.stride(1), *point, p(xb), p(yb), p(o["dA"]), p(o["dq"]), p(st), None),
        "ce_jvp_many": lambda: L.ce_jvp_many(eng._h, B, Kc, p(A_c), eng.nnz_aug, p(q_t), q_t.stride(0), q_t.stride(1), *point, *tang, p(o["dx"]), p(o["dy"]), p(o["ds"]), p(st), p(its),
                                             1e-8, 1e-8, 1e8, 0, None),
        "ce_jvp_qp_many": lambda: L.ce_jvp_qp_many(eng._h, B, Kc, p(A_c), eng.nnz_aug, p(P_c), *point, *tang, p(tP), tP.stride(0), nnzp, p(o["dx"]), p(o["dy"]), p(o["ds"]), p(st), p(its), None),
        "ce_vjp_qp_many": lambda: L.ce_vjp_qp_many(eng._h, B, Kc, p(A_c), eng.nnz_aug, p(P_c), *point, p(xb), p(yb), p(o["dA"]), p(o["dq"]), p(o["dP"]), p(st), None),
    }
    for who, call in calls.items():
        rc = call()
        msg = (L.ce_last_error() or b"").decode()
        assert rc == -2 and who in msg, (tag, who, rc, msg)
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in o.values()) and (st == 7).all() and (its == 7).all(), (tag, "a refused call wrote")
    return xb, yb, tA, tq, tP


def _as_the_single_calls(tag, what, many, single, Kc):
    """many() is torch.equal to the stacked single(k), or raises what single raises"""
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


def refused_case(name, shape):
    kind, n = shape[0], shape[1]
    tag = f"{name} ({kind}, n {n})"
    try:
        tpl, eng = _engine(shape)
    except (NotImplementedError, _lib.EngineError):
        assert pk.host_ns_plan(shape) is None, tag          # ce_create itself refuses the template: the host plan must, too
        print(f"{tag}: refused by ce_create")
        return
    host = _assert_plans_agree(name, shape, eng)
    L = _lib.lib()
    assert many_variant(kind, host) == -1, (tag, host)
    got = (L.ce_vjp_many_variant(eng._h), L.ce_jvp_many_variant(eng._h), L.ce_jvp_qp_many_variant(eng._h), L.ce_vjp_qp_many_variant(eng._h))
    assert got == (-1, -1, -1, -1), (tag, got)
    pt = K.plant(shape, **K.plant_args(name))
    dv = _device(pt, tpl, shape)
    Kc = 2
    xb, yb, tA, tq, tP = _raw_refusals(tag, eng, dv, pt, Kc)
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    A_bm = dv["A_bm"]
    if kind == "qp":
        kv = dict(path="per_instance", P_bm=dv["P_bm"])
        kj = dict(method="direct", P_bm=dv["P_bm"])
        _as_the_single_calls(tag, "vjp_many(qp_many=True)", lambda: eng.vjp_many(A_bm, x, y, s, xb, yb, qp_many=True, **kv),
                             lambda k: (lambda o: (o[0].t(), o[1].t(), o[2], o[3]))(eng.vjp(A_bm, x, y, s, xb[k], yb[k], **kv)), Kc)
        assert eng.last_vjp_many_path == "loop", tag
        _as_the_single_calls(tag, "jvp_many", lambda: eng.jvp_many(A_bm, x, y, s, tA, tq, tP=tP, **kj), lambda k: eng.jvp(A_bm, x, y, s, tA[k], tq[k].t(), tP_bm=tP[k], **kj), Kc)
    else:
        kv = dict(path="per_instance", lsqr=TIGHT_LSQR, q_eval=dv["q_t"])
        _as_the_single_calls(tag, "vjp_many", lambda: eng.vjp_many(A_bm, x, y, s, xb, yb, **kv),
                             lambda k: (lambda o: (o[0].t(), o[1].t(), o[2]))(eng.vjp(A_bm, x, y, s, xb[k], yb[k], **kv)), Kc)
        assert eng.last_vjp_many_path == "loop", tag
        _as_the_single_calls(tag, "jvp_many", lambda: eng.jvp_many(A_bm, x, y, s, tA, tq, method="direct", **kv),
                             lambda k: eng.jvp(A_bm, x, y, s, tA[k], tq[k].t(), method="direct", **kv), Kc)
    assert eng.last_jvp_many_path == "loop", tag


def run_group(group):
    cases = cases_of(group)
    assert cases, group
    recs = []
    for name, (shape, plan, what) in cases.items():
        if many_variant(shape[0], plan) >= 0:
            recs.append(served_case(name, shape))
        else:
            refused_case(name, shape)
    return recs


@pytest.mark.parametrize("group", GROUPS)
def test_many_modes_at_edges_and_structure_shapes(group):
    recs = run_group(group)
    assert recs, group
    if group.split(":")[0] in K.UNION_LARGEST:          # what the three union shapes are for: the member of the union region that qv2's rows must fit behind
        (rec,) = recs
        abc = pk.ns_union_members(rec["n"], rec["m"], rec["nq"], rec["row"])
        assert abc[K.UNION_LARGEST[group.split(":")[0]]] == max(abc), (group, abc)


def test_ledger_of_rows_and_many_modes():
    """one entry per (row of CE_NS_VARIANTS, many mode of csrc/ce_types.h) but the triples' (its ledger is tests/test_gpu_vjp_tri_many_edges.py): a new row or a
    new many mode fails here until a compared call at a shape with >= 80 % status-0 instances reaches it"""
    mine = [mode for by in MODES.values() for mode in by.values()]
    assert sorted(many_modes()) == sorted(mine + list(ELSEWHERE)), (many_modes(), "a many mode without an edge ledger")
    for group in GROUPS:
        if not all(name in _DONE for name, c in cases_of(group).items() if many_variant(c[0][0], c[1]) >= 0):
            run_group(group)
    reached = {}
    for rec in _DONE.values():
        for e in rec["reached"]:
            reached.setdefault(e, []).append(rec)
    below = [(r["name"], r[c + "_share"]) for r in _DONE.values() for c in ("adjoint", "jvp") if r[c + "_share"] < MIN_REGULAR]
    print("\nledger (row, mode, entry point): largest shape that reached it, status-0 share, largest error at a status-0 instance there; over all shapes of the kind: "
          "largest status-0 error, largest flagged error")
    missing = []
    for row in (r[0] for r in pk.variant_rows("CE_NS_VARIANTS")):
        for kind, by in MODES.items():
            for call, mode in by.items():
                if (row, mode) not in reached:
                    print(f"  row {row} {mode:12s} {ENTRY[mode]:15s} NOT REACHED"); missing.append((row, mode))
                    continue
                rec = max(reached[(row, mode)], key=lambda r: r["n"] * r["m"])
                every = [r for r in _DONE.values() if r["kind"] == kind]
                print(f"  row {row} {mode:12s} {ENTRY[mode]:15s} {rec['name']:28s} n {rec['n']:3d} m {rec['m']:4d} share {rec[call + '_share']:.3f} max {rec[call + '_max']:.2e}  "
                      f"({len(reached[(row, mode)])} shapes); all: status-0 {np.nanmax([r[call + '_max'] for r in every]):.2e} "
                      f"flagged {np.fmax.reduce([r[call + '_flagged'] for r in every]):.2e}")
    print("  shapes below the share:", below or "none")
    assert not missing, missing

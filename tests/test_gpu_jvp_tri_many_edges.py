"""The many-tangent forward derivative with exponential / power triples (k_backward_ns<..., FWD, ..., TRI, MANY> behind ce_jvp_tri_many) at the edges of the triples'
planner (csrc/ce_plan.h tri_ns_variant) and at the smallest shapes at which each part of the LDS layout exists: the `tri`-kind cases of ns_edge_kit.all_cases(),
at the planted KKT points and batch sizes of that kit (tests/test_ns_edge_kit.py proves every instance regular without a GPU).

The mode is an object of its own, not a mode of csrc/ce_tu_ns.hip, and its argument struct is named NsJvpManyTri so that the ledger of
tests/test_gpu_ns_many_edges.py (which collects the Ns...Many overloads of ce_types.h) keeps its five names; this file is the mode's own ledger
(tests/test_jvp_tri_many_args.py pins both).
At each served shape, K = 3 (a Gaussian tangent, the zero tangent, the first one again), with the references and bounds test_gpu_ns_mode_edges.py holds NsJvpTri to:
  * the library's variant equals the host plan's tri_ns_variant;
  * every status-0 instance matches the dense solve at the planted point (ns_edge_kit.dense_jvp) within 1e-5 relative to 1 + max |reference|, no iteration; a
    flagged instance (4 | 8) is re-solved by LSQR under TIGHT_LSQR: median 1e-6, maximum 5e-3 -- flagged instances are not excused;
  * the zero tangent gives exact zeros on status-0 instances, the repeat is bit-identical;
  * a shape counts for the ledger when >= 80 % of its instances have status 0.
On the first refused shape: CE_E_UNSUPPORTED with the outputs untouched, and jvp_many(tri_many=True) runs the loop.
Ledger: every row of CE_NS_VARIANTS must be reached by a compared call."""
import numpy as np
import pytest
import torch

import ns_edge_kit as K
import plan_kit as pk
from cvxpylayers_amd import _lib
from kit import TIGHT_LSQR
from test_gpu_ns_mode_edges import MIN_REGULAR, _device, _engine, _rel

pytestmark = pytest.mark.gpu

_DONE: dict = {}
KC = 3
KW = dict(method="direct", path="per_instance", lsqr=TIGHT_LSQR)


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for e in pk.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)


def tri_cases(group=None):
    every = {k: c for k, c in K.all_cases().items() if c[0][0] == "tri"}
    return every if group is None else {k: c for k, c in every.items() if k == group or k.startswith(group + "[")}


GROUPS = [f for f in pk.NS_FAMILIES if pk.NS_FAMILIES[f][0] == "tri"] + [f"{name}:tri" for name, by in K.STRUCTURE.items() if "tri" in by]


def served_case(name, shape):
    if name in _DONE:
        return _DONE[name]
    n = shape[1]
    pt = K.point(name, shape, **K.plant_args(name))
    cond, resid = K.regularity(pt)
    assert (cond <= 1e11).all() and (resid <= 1e-13).all(), (name, cond, resid)
    tpl, eng = _engine(shape)
    host = pk.host_ns_plan(shape)
    row = host["tri_ns_variant"]
    L = _lib.lib()
    assert row >= 0 and L.ce_jvp_tri_many_variant(eng._h) == row == L.ce_tri_ns_variant(eng._h), (name, host, L.ce_jvp_tri_many_variant(eng._h))
    assert L.ce_jvp_many_variant(eng._h) == -1, name
    dv = _device(pt, tpl, shape)
    B, m = pt["x"].shape[0], pt["m"]
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    tag = f"{name} (n {n}, m {m}, B {B}, row {row})"
    t = K.tangents(pt)
    tA_eval, tq_eval = tpl.values_from_dense(*t[:3])
    tA = np.zeros((KC, B, eng.nnz_aug)); tq = np.zeros((KC, B, n + 1))
    tA[0] = tA[2] = tA_eval.T; tq[0] = tq[2] = tq_eval.T
    got = eng.jvp_many(dv["A_bm"], x, y, s, torch.from_numpy(tA).cuda(), torch.from_numpy(tq).cuda(), q_eval=dv["q_t"], tri_many=True, **KW)
    assert eng.last_jvp_many_path == "many" and eng.last_jvp_kernel == "ce_jvp_tri_many", tag
    torch.cuda.synchronize()
    dx, dy, ds, st = (g.cpu().numpy() for g in got); its = eng.last_lsqr_iters.cpu().numpy()
    assert ((st & (4 | 8)) == (st[:1] & (4 | 8))).all() and ((st & 3) == 0).all() and ((st == 0) | ((st & 12) == 12)).all(), (tag, st)
    want = K.dense_jvp(pt, t)
    assert want[3].all(), tag          # no instance left out on the reference's account
    reg = st[0] == 0
    fl = ~reg
    rec = dict(name=name, n=n, m=m, B=B, row=row, share=float(reg.mean()), reached=False)
    for k in (0, 2):
        e = np.max([_rel(g[k], w) for g, w in zip((dx, dy, ds), want[:3])], axis=0)
        print(f"{tag} k={k}: status-0 share {reg.mean():.3f} status counts {np.bincount(st[k]).tolist()} error max {e.max():.3e}" +
              (f", status-0 max {e[reg].max():.3e} median {np.median(e[reg]):.3e}" if reg.any() else "") + (f", flagged {e[fl].tolist()}" if fl.any() else ""))
        if reg.any():
            assert e[reg].max() < 1e-5, (tag, k, e[reg].max())
            assert (its[k][reg] == 0).all(), (tag, k, its[k])
        if fl.any():          # flagged instances are not excused
            assert (st[k][fl] == 12).all() and (its[k][fl] > 0).all(), (tag, k, st[k], its[k])
            assert np.median(e[fl]) < 1e-6 and e[fl].max() < 5e-3, (tag, k, e[fl])
        rec[f"err{k}"] = float(e[reg].max()) if reg.any() else float("nan")
    for g in (dx, dy, ds):
        assert (g[1][reg] == 0).all() and np.isfinite(g).all(), (tag, "the zero tangent")
        assert np.array_equal(g[0], g[2]), (tag, "the repeated tangent")
    rec["reached"] = bool(reg.mean() >= MIN_REGULAR)
    if not rec["reached"]:
        print(f"{tag}: status-0 share {reg.mean():.3f} below {MIN_REGULAR}: NOT counted as coverage")
    _DONE[name] = rec
    return rec


def refused_case(name, shape):
    n = shape[1]
    tag = f"{name} (n {n})"
    try:
        tpl, eng = _engine(shape)
    except (NotImplementedError, _lib.EngineError):
        assert pk.host_ns_plan(shape) is None, tag          # ce_create itself refuses the template: the host plan must, too
        print(f"{tag}: refused by ce_create")
        return
    host = pk.host_ns_plan(shape)
    L = _lib.lib()
    assert host["tri_ns_variant"] == -1 and L.ce_jvp_tri_many_variant(eng._h) == -1, (tag, host)
    pt = K.plant(shape, **K.plant_args(name))
    dv = _device(pt, tpl, shape)
    B, Kc, m = pt["x"].shape[0], 2, pt["m"]
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    rng = np.random.default_rng(pt["seed"] + 31)
    tA = torch.from_numpy(rng.standard_normal((Kc, B, eng.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((Kc, B, n + 1))).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    dx = torch.full((Kc, B, n), 7.0, **f64); dy = torch.full((Kc, B, m), 7.0, **f64); ds = torch.full((Kc, B, m), 7.0, **f64)
    st = torch.full((Kc, B), 7, dtype=torch.int32, device="cuda"); its = torch.full((Kc, B), 7, dtype=torch.int32, device="cuda")
    A_c = dv["A_bm"].contiguous(); q_t = dv["q_t"]
    rc = L.ce_jvp_tri_many(eng._h, B, Kc, A_c.data_ptr(), eng.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                           tA.data_ptr(), tA.stride(0), eng.nnz_aug, tq.data_ptr(), tq.stride(0), n + 1, dx.data_ptr(), dy.data_ptr(), ds.data_ptr(), st.data_ptr(), its.data_ptr(),
                           1e-8, 1e-8, 1e8, 0, None)
    msg = (L.ce_last_error() or b"").decode()
    torch.cuda.synchronize()
    assert rc == -2 and "ce_jvp_tri_many" in msg, (tag, rc, msg)
    assert (dx == 7.0).all() and (dy == 7.0).all() and (ds == 7.0).all() and (st == 7).all() and (its == 7).all(), (tag, "a refused call wrote")
    try:
        got = eng.jvp_many(dv["A_bm"], x, y, s, tA, tq, q_eval=q_t, tri_many=True, **KW)
    except _lib.EngineError as e:          # (a shape ce_jvp itself refuses: the loop is the flag's fall-back, and it says what ce_jvp says)
        assert eng.last_jvp_many_path == "loop", tag
        print(f"{tag}: ce_jvp_tri_many refused ({msg}); jvp_many(tri_many=True) took the loop, which ce_jvp refuses: {e}")
        return
    assert eng.last_jvp_many_path == "loop" and eng.last_jvp_kernel != "ce_jvp_tri_many", tag
    torch.cuda.synchronize()
    assert got[0].shape == (Kc, B, n) and torch.isfinite(got[0]).all(), tag
    print(f"{tag}: ce_jvp_tri_many refused ({msg}); jvp_many(tri_many=True) ran the loop ({eng.last_jvp_kernel})")


def run_group(group):
    cases = tri_cases(group)
    assert cases, group
    recs = []
    for name, (shape, plan, what) in cases.items():
        if pk.ns_served("tri", plan):
            recs.append(served_case(name, shape))
        else:
            refused_case(name, shape)
    return recs


@pytest.mark.parametrize("group", GROUPS)
def test_the_mode_at_edges_and_structure_shapes(group):
    assert run_group(group), group


def test_every_row_is_reached_by_a_compared_call():
    for group in GROUPS:
        if not all(name in _DONE for name, c in tri_cases(group).items() if pk.ns_served("tri", c[1])):
            run_group(group)
    rows = [r[0] for r in pk.variant_rows("CE_NS_VARIANTS")]
    print("\nledger of ce_jvp_tri_many / NsJvpManyTri (row: largest shape that reached it, status-0 share, error of the first tangent)")
    missing = []
    for row in rows:
        recs = [r for r in _DONE.values() if r["row"] == row and r["reached"]]
        if not recs:
            print(f"  row {row} NOT REACHED"); missing.append(row)
            continue
        r = max(recs, key=lambda q: q["n"] * q["m"])
        print(f"  row {row} {r['name']:28s} n {r['n']:3d} m {r['m']:4d} share {r['share']:.3f} max {r['err0']:.2e}  ({len(recs)} shapes)")
    assert not missing, missing

"""The many-cotangent adjoint with exponential / power triples (k_backward_ns<..., TRI, MANY> without FWD behind ce_vjp_tri_many) at the edges of the triples'
planner (csrc/ce_plan.h tri_ns_variant) and at the smallest shapes at which each part of the LDS layout exists: the `tri`-kind cases of ns_edge_kit.all_cases(),
at the planted KKT points and batch sizes of that kit (tests/test_ns_edge_kit.py proves every instance regular without a GPU).

The mode is an object of its own, not a mode of csrc/ce_tu_ns.hip, so tests/test_gpu_ns_mode_edges.py's ledger does not see it; this file keeps the mode's own.
At each served shape, K = 3 (a Gaussian cotangent, the zero cotangent, the first one again):
  * the library's variant equals the host plan's tri_ns_variant;
  * every status-0 instance matches the oracle's dense elimination at the planted point within 1e-5 relative to 1 + max |reference|; a flagged instance (4 | 8) is
    re-solved by LSQR under TIGHT_LSQR and held to the flagged bound of test_gpu_ns_mode_edges.py (median 1e-6, maximum 5e-3) -- flagged instances are not excused;
  * the transpose identity against ce_jvp holds where both report status 0;
  * a shape counts for the ledger when >= 80 % of its instances have status 0 (the rule of test_gpu_ns_mode_edges.py).
On the first refused shape: CE_E_UNSUPPORTED with the outputs untouched, and vjp_many(tri_many=True) runs the loop.
Ledger: every row of CE_NS_VARIANTS must be reached by a compared call."""
import numpy as np
import pytest
import torch

import ns_edge_kit as K
import plan_kit as pk
from cvxpylayers_amd import _lib
from kit import TIGHT_LSQR
from test_gpu_ns_mode_edges import MIN_REGULAR, _boundary, _device, _engine, _rel

pytestmark = pytest.mark.gpu

_DONE: dict = {}
KC = 3


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
    from oracle import oracle
    n = shape[1]
    pt = K.point(name, shape, **K.plant_args(name))
    cond, resid = K.regularity(pt)
    assert (cond <= 1e11).all() and (resid <= 1e-13).all(), (name, cond, resid)
    tpl, eng = _engine(shape)
    host = pk.host_ns_plan(shape)
    row = host["tri_ns_variant"]
    L = _lib.lib()
    assert row >= 0 and L.ce_vjp_tri_many_variant(eng._h) == row == L.ce_tri_ns_variant(eng._h), (name, host, L.ce_vjp_tri_many_variant(eng._h))
    assert L.ce_vjp_many_variant(eng._h) == -1 and L.ce_adjoint_ns_variant(eng._h) == -1, name
    dv = _device(pt, tpl, shape)
    B, m = pt["x"].shape[0], pt["m"]
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    tag = f"{name} (n {n}, m {m}, B {B}, row {row})"
    rng = np.random.default_rng(pt["seed"] + 31)
    xb = np.zeros((KC, B, n)); yb = np.zeros((KC, B, m))
    xb[0] = xb[2] = rng.standard_normal((B, n)); yb[0] = yb[2] = rng.standard_normal((B, m))
    dA, dq, adj = eng.vjp_many(dv["A_bm"], x, y, s, torch.from_numpy(xb).cuda(), torch.from_numpy(yb).cuda(), path="per_instance", lsqr=TIGHT_LSQR, q_eval=dv["q_t"], tri_many=True)
    assert eng.last_vjp_many_path == "many" and eng.last_vjp_kernel == "ce_vjp_tri_many", tag
    torch.cuda.synchronize()
    dA, dq, adj = dA.cpu().numpy(), dq.cpu().numpy(), adj.cpu().numpy()
    assert ((adj & (4 | 8)) == (adj[:1] & (4 | 8))).all() and ((adj & 3) == 0).all() and ((adj == 0) | ((adj & 12) == 12)).all(), (tag, adj)
    g = oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], pt["cones"], pt["x"], pt["y"], pt["s"], xb[0], yb[0], mode="dense")
    wantA = _boundary(tpl, g, n).T
    reg = adj[0] == 0
    rec = dict(name=name, n=n, m=m, B=B, row=row, share=float(reg.mean()), reached=False)
    for k in (0, 2):
        e = np.maximum(_rel(dA[k], wantA), _rel(dq[k][:, :n], g["dc"]))
        print(f"{tag} k={k}: status-0 share {reg.mean():.3f} status counts {np.bincount(adj[k]).tolist()} error max {e.max():.3e}" +
              (f", status-0 max {e[reg].max():.3e}" if reg.any() else "") + (f", flagged {e[~reg].tolist()}" if (~reg).any() else ""))
        if reg.any():
            assert e[reg].max() < 1e-5, (tag, k, e[reg].max())
        if (~reg).any():
            assert np.median(e[~reg]) < 1e-6 and e[~reg].max() < 5e-3, (tag, k, e[~reg])
        assert (dq[k][:, n] == 0).all()
        rec[f"err{k}"] = float(e[reg].max()) if reg.any() else float("nan")
    assert (dA[1][reg] == 0).all() and (dq[1][reg] == 0).all(), (tag, "the zero cotangent")
    assert np.isfinite(dA).all() and np.isfinite(dq).all(), tag
    # the transpose identity against the forward derivative of the same elimination
    t = K.tangents(pt)
    tA_eval, tq_eval = tpl.values_from_dense(*t[:3])
    tA_bm, tq = torch.from_numpy(tA_eval).cuda().t().contiguous(), torch.from_numpy(tq_eval).cuda()
    dx, dy, ds, st = eng.jvp(dv["A_bm"], x, y, s, tA_bm, tq, method="direct", path="per_instance", lsqr=TIGHT_LSQR, q_eval=dv["q_t"])
    assert eng.last_jvp_kernel == "ce_jvp", tag
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert ((st & 4) == (adj[0] & 4)).all(), (tag, st, adj[0])          # the same elimination flags the same instances
    both = (st == 0) & reg
    if both.any():
        lhs = (xb[0] * dx.cpu().numpy()).sum(axis=1) + (yb[0] * dy.cpu().numpy()).sum(axis=1)
        rhs = (dA[0] * tA_bm.cpu().numpy()).sum(axis=1) + (dq[0] * tq.cpu().numpy().T).sum(axis=1)
        ti = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
        print(f"{tag} transpose identity: max {ti[both].max():.3e}")
        assert (ti[both] < 1e-6).all() and np.abs(lhs[both]).max() > 1e-3, (tag, ti)
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
    assert host["tri_ns_variant"] == -1 and L.ce_vjp_tri_many_variant(eng._h) == -1, (tag, host)
    pt = K.plant(shape, **K.plant_args(name))
    dv = _device(pt, tpl, shape)
    B, Kc = pt["x"].shape[0], 2
    x, y, s = (torch.from_numpy(pt[k]).cuda() for k in "xys")
    rng = np.random.default_rng(pt["seed"] + 31)
    xb = torch.from_numpy(rng.standard_normal((Kc, B, n))).cuda(); yb = torch.from_numpy(rng.standard_normal((Kc, B, pt["m"]))).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    dA = torch.full((Kc, B, eng.nnz_aug), 7.0, **f64); dq = torch.full((Kc, B, n + 1), 7.0, **f64); st = torch.full((Kc, B), 7, dtype=torch.int32, device="cuda")
    A_c = dv["A_bm"].contiguous(); q_t = dv["q_t"]
    rc = L.ce_vjp_tri_many(eng._h, B, Kc, A_c.data_ptr(), eng.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                           xb.data_ptr(), yb.data_ptr(), dA.data_ptr(), dq.data_ptr(), st.data_ptr(), None)
    msg = (L.ce_last_error() or b"").decode()
    torch.cuda.synchronize()
    assert rc == -2 and "ce_vjp_tri_many" in msg, (tag, rc, msg)
    assert (dA == 7.0).all() and (dq == 7.0).all() and (st == 7).all(), (tag, "a refused call wrote")
    got = eng.vjp_many(dv["A_bm"], x, y, s, xb, yb, path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t, tri_many=True)
    assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None, tag
    torch.cuda.synchronize()
    assert got[0].shape == (Kc, B, eng.nnz_aug) and torch.isfinite(got[0]).all(), tag
    print(f"{tag}: ce_vjp_tri_many refused ({msg}); vjp_many(tri_many=True) ran the loop")


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
    print("\nledger of ce_vjp_tri_many (row: largest shape that reached it, status-0 share, error of the first cotangent)")
    missing = []
    for row in rows:
        recs = [r for r in _DONE.values() if r["row"] == row and r["reached"]]
        if not recs:
            print(f"  row {row} NOT REACHED"); missing.append(row)
            continue
        r = max(recs, key=lambda q: q["n"] * q["m"])
        print(f"  row {row} {r['name']:28s} n {r['n']:3d} m {r['m']:4d} share {r['share']:.3f} max {r['err0']:.2e}  ({len(recs)} shapes)")
    assert not missing, missing

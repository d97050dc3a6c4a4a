"""Every kernel variant at the edges of its launch plan (include/cone_engine.h ce_get_plan).

Discovery: for every template family of plan_kit, engines are created (no solve) over the swept size in steps of 1 and the sizes where the plan changes are
kept, the last before and the first after each change; edges are deduplicated by their (plan before, plan after) pair over all families.
Parity at each edge shape, both sides, against the CPU oracle on seeded strictly feasible data (B = 37; 12 when n m > 6000):
  * forward at eps 1e-9, acceleration off: statuses equal, x / y / s within 1e-6 (1 + |.|inf); with the one-pair acceleration on both sides where aa_ok;
  * every adjoint kernel the plan offers at the oracle's point, against the oracle's dense elimination within 1e-5 relative: ce_vjp with q_eval (k_backward_ns +
    LSQR re-solve), without it (k_backward_rt / size-generic), and a second call of the same batch size for the two-tile plan; the smallest first tile
    the two-tile plan may use, forced on an engine of its own, bit-identical to the single tile (and variant 4, which only m < n templates plan, forced);
  * the native quadratic objective: ce_solve_qp / ce_vjp_qp (dP too) against the oracle given P;
  * shared-A templates: the shared-A path (CE_CONST_A=1: k_sa_* at sp_RP 16 / 32 / 64, the batch-GEMM fallback at 0) against the oracle's solution and its
    LSQR adjoint under the same tight rule;
  * every row of the shared-A kernels' lists (csrc/ce_variants.h CE_SA_FWD_VARIANTS, CE_SA_LSQR_VARIANTS) on the shared family at 3 / 20 / 40 dense rows with
    nonnegative rows only, plus a PSD block of order 3, plus an exponential triple (B = 5): the row ce_get_plan reports after the call (last_sa_fwd,
    last_sa_lsqr) is the one the cones and the call-time switches ask for, and the call's results are the oracle's (sa_rows_at).
Coverage ledger: the plans reached (default planning over the sweeps, plus the create-time switches on the edge shapes) cover every instantiated variant; a
row of the shared-A lists counts as reached only through such a compared call."""
import numpy as np
import pytest
import torch

import plan_kit as pk
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR

pytestmark = pytest.mark.gpu

EPS, MAX_IT = 1e-9, 400000          # (pure LPs converge slowly under operator splitting: tens of thousands of iterations)
_CACHE = {}


def discovery():
    """{family: [values of its retained edge shapes]}, all plans seen {key: (family, v, plan)}, the deduplicated edges"""
    if "d" in _CACHE:
        return _CACHE["d"]
    edges, seen = [], {}
    for fam in pk.all_families(ledger=True):
        def fn(v, fam=fam):
            p = pk.plan_of(fam, v)
            if p is not None:
                seen.setdefault(pk.key(p), (fam, v, p))
            return p
        es = pk.find_edges(fn, pk.family_values(fam), fields=pk.fields_for(fam))
        if fam not in pk.LEDGER_FAMILIES:
            edges += [(fam,) + e for e in es]
    kept, pairs = [], set()
    for fam, vb, pb, va, pa in edges:
        k = (pk.key(pb, pk.fields_for(fam)), pk.key(pa, pk.fields_for(fam)))
        if k not in pairs:
            pairs.add(k)
            kept.append((fam, vb, pb, va, pa))
    shapes = {}
    for fam, vb, pb, va, pa in kept:
        for v, p in ((vb, pb), (va, pa)):
            if p is not None and v not in shapes.setdefault(fam, []):
                shapes[fam].append(v)
    _CACHE["d"] = (shapes, seen, kept)
    print(f"\nplan discovery: {len(edges)} edges, {len(kept)} after deduplication, {sum(len(v) for v in shapes.values())} edge shapes")
    for fam, vb, pb, va, pa in kept:
        diff = {f: (pb[f] if pb else None, pa[f] if pa else None) for f in pk.fields_for(fam) if (pb or {}).get(f) != (pa or {}).get(f)}
        print(f"  {fam}: {vb} -> {va}  {diff}")
    return _CACHE["d"]


# --------------------------------------------------------------------------------------------------------- coverage ledger
def variants_of(p, fam):
    """the ledger entries a plan reaches (sp_RP: on shared-A templates only -- the k_sa_* kernels serve nothing else)"""
    out = []
    if p["fwd_mode"] == 4:
        out.append(f"fwd k_fwd2 v{p['f2_variant']}" + (" +P" if p["qp_native"] else "") + (" WL" if p["wl"] else "") + (" AA" if p["aa_ok"] else ""))
        out += [f"fwd k_fwd2 v{p['f2_variant']}", f"fwd k_fwd2 WL={p['wl']}", f"fwd k_fwd2 aa_ok={p['aa_ok']}"]
        if p["qp_native"]:
            out.append(f"fwd k_fwd2 v{p['f2_variant']} +P")
    elif p["fwd_mode"] == 3:
        out.append(f"fwd k_forward_rt v{p['rt_variant']}")
    else:
        out.append(f"fwd generic mode {p['fwd_mode']} blocked={p['gen_blocked_f']}")
    if p["ns_variant"] >= 0:
        out.append(f"bwd k_backward_ns v{p['ns_variant']}")
    if p["bwd_mode"] == 3:
        out.append(f"bwd k_backward_rt v{p['brt_variant']}")
        if p["two_tile"]:
            out.append("bwd two-tile plan")
    else:
        out.append(f"bwd generic mode {p['bwd_mode']} blocked={p['gen_blocked_b']}")
    if fam == pk.SHARED_FAMILY[0]:
        out.append(f"shared-A sp_RP={p['sp_RP']}")
    return out


def sa_fwd_name(RP, NTH, CIDX, HTRI):
    return f"k_sa_fwd RP={RP} NTH={NTH} CIDX={CIDX} HTRI={HTRI}"


def sa_lsqr_name(RP, HPSD, HTRI, LSMR, FWD):
    return f"k_sa_lsqr RP={RP} HPSD={HPSD} HTRI={HTRI} LSMR={LSMR} FWD={FWD}"


EXPECTED = ([f"fwd k_fwd2 v{v}" for v in range(5)] + [f"fwd k_fwd2 v{v} +P" for v in (2, 3, 4)] + ["fwd k_fwd2 WL=0", "fwd k_fwd2 WL=1", "fwd k_fwd2 aa_ok=0", "fwd k_fwd2 aa_ok=1"]
            + [f"fwd k_forward_rt v{v}" for v in range(3)] + ["fwd generic mode 0 blocked=0"] + [f"fwd generic mode {m} blocked={b}" for m in (1, 2) for b in (0, 1)]
            + [f"bwd k_backward_ns v{v}" for v in range(3)] + [f"bwd k_backward_rt v{v}" for v in range(7)] + ["bwd two-tile plan"]
            + ["bwd generic mode 0 blocked=0"] + [f"bwd generic mode {m} blocked={b}" for m in (1, 2) for b in (0, 1)]
            + [f"shared-A sp_RP={r}" for r in (16, 32, 64, 0)]
            + [sa_fwd_name(*r[1:]) for r in pk.variant_rows("CE_SA_FWD_VARIANTS")] + [sa_lsqr_name(*r[1:]) for r in pk.variant_rows("CE_SA_LSQR_VARIANTS")])
# variants no shape or switch can reach, with the reason
EXPECTED_UNREACHABLE = {
    "fwd k_fwd2 aa_ok=0": "the largest k_fwd2 footprint (variant 4 at its largest n, m, PSD block and P) is 122 KB with the five Anderson vectors, "
                          "below the 160 KiB LDS limit: every template k_fwd2 serves carries them (asserted on every k_fwd2 plan discovery meets)",
}

SWITCHES = [{}, {"CE_FWD": "rt"}, {"CE_FWD": "generic"}, {"CE_FORCE_GENERIC": "1"}, {"CE_BWD_NS": "0"}, {"CE_GEN_BLOCKED": "0"}, {"CE_WL": "0"},
            {"CE_FORCE_GENERIC": "1", "CE_GEN_BLOCKED": "0"}]


def test_coverage_ledger(monkeypatch):
    shapes, seen, kept = discovery()
    ledger = {}
    no_aa = [(fam, v) for fam, v, p in seen.values() if p["fwd_mode"] == 4 and not p["aa_ok"]]
    assert not no_aa, f"k_fwd2 plans without the Anderson vectors: {no_aa} (EXPECTED_UNREACHABLE is wrong)"
    for k, (fam, v, p) in seen.items():
        for var in variants_of(p, fam):
            ledger.setdefault(var, f"{fam} v={v} {pk.shape_of(fam, v)[:2]}")
    for sw in SWITCHES[1:]:
        with monkeypatch.context() as mp:
            for e, val in sw.items():
                mp.setenv(e, val)
            for fam, vals in shapes.items():
                for v in vals:
                    p = pk.plan_of(fam, v)
                    if p is not None:
                        for var in variants_of(p, fam):
                            ledger.setdefault(var, f"{fam} v={v} {pk.shape_of(fam, v)[:2]} under {sw}")
    for RP in SA_V:
        for fam in pk.SHARED_CONE_SETS:
            for var, where in sa_rows_at(RP, fam, monkeypatch).items():
                ledger.setdefault(var, where)
    missing = []
    print("\ncoverage ledger:")
    for var in EXPECTED:
        where = ledger.get(var) or (f"expected unreachable: {EXPECTED_UNREACHABLE[var]}" if var in EXPECTED_UNREACHABLE else None)
        print(f"  {var:50s} {where or 'NOT REACHED'}")
        if where is None:
            missing.append(var)
    assert not missing, missing


# --------------------------------------------------------------------------------------------------------- parity
def _boundary(tpl, g, n):
    cols = np.repeat(np.arange(n + 1), np.diff(tpl.indptr))
    return np.stack([-g["dA"][:, i, j] if j < n else g["db"][:, i] for i, j in zip(tpl.indices, cols)])


def _rel(got, want):
    return float((np.abs(got - want).max(axis=-1) / (1 + np.abs(want).max(axis=-1))).max())


def _data(fam, v, B, seed):
    n, cones, pat, pstruct = pk.shape_of(fam, v)
    m = P.cone_rows(cones)
    if pat is not None:          # shared A: one matrix for the batch, bound rows -(0.5 .. 1.5) on the variables
        rng = np.random.default_rng(seed)
        A0 = np.where(pat, rng.standard_normal(pat.shape) / np.sqrt(n), 0.0)
        A0[cones["l"] - n + np.arange(n), np.arange(n)] = -(0.5 + rng.random(n))
        x0 = rng.standard_normal((B, n)) * 0.5; s0, y0 = P._interior_point(rng, cones, B)
        A = np.broadcast_to(A0, (B, m, n)).copy(); b = x0 @ A0.T + s0; c = -(y0 @ A0)
    else:
        A, b, c = P.generate(n, cones, B, seed=seed)
    Pm = None
    if pstruct is not None:
        rng = np.random.default_rng(seed + 5)
        F = rng.standard_normal((B, n, n)) / np.sqrt(n)
        Pm = F @ F.transpose(0, 2, 1) + 0.1 * np.eye(n)
    return n, m, cones, pat, pstruct, A, b, c, Pm


# k_backward_rt tiles {TI, TJ, TH, BGR} (csrc/ce_variants.h CE_BRT_VARIANTS)
BRT = [(4, 4, 4, 16), (5, 5, 4, 16), (6, 6, 4, 16), (7, 7, 4, 16), (7, 7, 7, 16), (5, 9, 7, 32), (7, 13, 7, 32)]


def first_tiles(brt):
    """the first tiles the two-tile plan may choose for a worst-case tile brt: those that differ from it in TI / TJ alone (bit-identical gradients)"""
    return [v for v in range(brt) if BRT[v][2:] == BRT[brt][2:]]


def _oracle_data(fam, v, B, seed, native_p):
    """_data and the oracle's solution of it; an instance at which the oracle itself does not converge is replaced by a reseeded one, not skipped (shared A: the
    whole batch, whose A it shares)"""
    from oracle import oracle
    n, m, cones, pat, pstruct, A, b, c, Pm = _data(fam, v, B, seed)
    if not native_p:
        Pm = None
    ref = oracle.solve_batch(A, b, c, cones, eps=EPS, max_iters=MAX_IT, P=Pm)
    for attempt in range(1, 7):
        bad = np.flatnonzero(ref["status"] != 1)
        if len(bad) == 0:
            break
        if pat is not None:
            bad = np.arange(B)
        _, _, _, _, _, A2, b2, c2, P2 = _data(fam, v, len(bad), seed + 1000 * attempt)
        A[bad], b[bad], c[bad] = A2, b2, c2
        if Pm is not None:
            Pm[bad] = P2
        r2 = oracle.solve_batch(A2, b2, c2, cones, eps=EPS, max_iters=MAX_IT, P=None if Pm is None else P2)
        for k in ref:
            ref[k][bad] = r2[k]
    else:
        pytest.fail(f"{fam} v={v}: the oracle does not converge on {len(bad)} instances after six reseeds")
    return n, m, cones, pat, pstruct, A, b, c, Pm, ref


def parity_at(fam, v, monkeypatch, seed=0, force=()):
    """force: first tiles to force (CE_BWD_FAST_VARIANT) on engines of their own, besides the smallest one the two-tile plan may choose by itself"""
    from oracle import oracle
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings
    n0, cones0, _, pstruct0 = pk.shape_of(fam, v)
    m0 = P.cone_rows(cones0)
    B = 37 if n0 * m0 <= 6000 else 12
    dev = torch.device("cuda", 0)
    tpl = P.dense_template(n0, cones0, pattern=pk.shape_of(fam, v)[2])
    eng = ConeEngine(tpl.indices, tpl.indptr, n0, m0, cones0, dev, p_structure=pstruct0)
    plan = eng.plan()
    native_p = pstruct0 is not None and eng.qp_native      # (a P structure the kernels cannot hold is the plugin's epigraph form: the engine serves the linear objective)
    n, m, cones, pat, pstruct, A, b, c, Pm, ref = _oracle_data(fam, v, B, seed, native_p)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    A_bm = eng.to_batch_major(torch.from_numpy(A_eval).to(dev)); q_t = torch.from_numpy(q_eval).to(dev)
    P_bm = None
    if native_p:
        idx, ptr = pstruct
        pc = np.repeat(np.arange(n), np.diff(ptr))
        P_bm = torch.from_numpy(np.ascontiguousarray(Pm[:, idx, pc])).to(dev)
    else:
        pstruct = None
    tag = f"{fam} v={v} n={n} m={m} plan={ {k: plan[k] for k in pk.EDGE_FIELDS} }"
    shared = pat is not None
    with monkeypatch.context() as mp:
        if shared:
            mp.setenv("CE_CONST_A", "1")
        x, y, s, iters, status, _ = eng.solve(A_bm, q_t, make_settings(dict(eps=EPS, max_iters=MAX_IT, acceleration_lookback=0)), P_bm=P_bm)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == ref["status"]).all(), (tag, status.cpu().numpy())
        for nm, got, want in (("x", x, ref["x"]), ("y", y, ref["y"]), ("s", s, ref["s"])):
            assert _rel(got.cpu().numpy(), want) < 1e-6, (tag, nm, _rel(got.cpu().numpy(), want))
        if plan["aa_ok"] and not shared:
            ra = oracle.solve_batch(A, b, c, cones, eps=EPS, max_iters=MAX_IT, P=Pm, aa_mem=1)
            xa, _, _, _, sta, _ = eng.solve(A_bm, q_t, make_settings(dict(eps=EPS, max_iters=MAX_IT, acceleration_lookback=1)), P_bm=P_bm)
            torch.cuda.synchronize()
            ok = ra["status"] == 1
            assert (sta.cpu().numpy()[ok] == 1).all(), (tag, "accelerated", sta.cpu().numpy(), ra["status"])
            assert _rel(xa.cpu().numpy()[ok], ra["x"][ok]) < 1e-6, (tag, "accelerated x")
        rng = np.random.default_rng(seed + 7)
        dx = rng.standard_normal((B, n)); dy = rng.standard_normal((B, m))
        xr, yr, sr, dxt, dyt = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (ref["x"], ref["y"], ref["s"], dx, dy))
        if shared:
            g = oracle.adjoint_batch(A, b, c, cones, ref["x"], ref["y"], ref["s"], dx, dy, mode="lsqr",
                                     lsqr_atol=TIGHT_LSQR[0], lsqr_btol=TIGHT_LSQR[1], lsqr_iter_lim=TIGHT_LSQR[2])
            calls = [("shared-A LSQR", dict(path="const_a", lsqr=TIGHT_LSQR, q_eval=q_t))]
        else:
            g = oracle.adjoint_batch(A, b, c, cones, ref["x"], ref["y"], ref["s"], dx, dy, P=Pm, mode="dense")
            if pstruct is not None:
                calls = [("qp", dict(P_bm=P_bm))]
            else:
                calls = [("elimination", dict(path="per_instance_dense")),
                         ("q_eval (ns / re-solve)", dict(path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t))]
                if plan["two_tile"]:
                    calls.append(("two-tile second call", dict(path="per_instance_dense")))
        want = _boundary(tpl, g, n)
        single = None
        for what, kw in calls:
            out = eng.vjp(A_bm, xr, yr, sr, dxt, dyt, **kw)
            torch.cuda.synchronize()
            dA, dq, adj = out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy()
            assert ((adj & 3) == 0).all(), (tag, what, adj)
            assert _rel(dA.T, want.T) < 1e-5, (tag, what, "dA", _rel(dA.T, want.T))
            assert _rel(dq[:n].T, g["dc"]) < 1e-5, (tag, what, "dc")
            assert np.abs(dq[n]).max() == 0
            if pstruct is not None:
                idx, ptr = pstruct
                pc = np.repeat(np.arange(n), np.diff(ptr))
                wantP = g["dP"][:, idx, pc] + np.where(idx != pc, g["dP"][:, pc, idx], 0.0)
                assert _rel(out[3].cpu().numpy(), wantP) < 1e-5, (tag, "dP")
            if what == "elimination":
                assert eng.plan()["last_fast"] == -1          # (an engine's first call has no history: the worst-case tile alone)
                single = (out[0].clone(), out[1].clone(), out[2].clone())
            if what == "two-tile second call":
                lf = eng.plan()["last_fast"]
                print(f"  {tag}: two-tile first tile chosen from the previous call: {lf}")
                if lf >= 0:
                    assert all(torch.equal(a_, b_) for a_, b_ in zip(out[:3], single)), (tag, "two-tile plan not bit-identical to the single tile")
        # the first tiles themselves, forced (the history above may leave no smaller tile that holds the largest system)
        forced = list(force) + (first_tiles(plan["brt_variant"])[:1] if plan["two_tile"] and not shared and pstruct is None else [])
        for fv in forced:
            mp.setenv("CE_BWD_FAST_VARIANT", str(fv))
            engf = ConeEngine(tpl.indices, tpl.indptr, n, m, cones, dev)
            mp.delenv("CE_BWD_FAST_VARIANT")
            assert engf.plan()["two_tile"] == 1, tag
            for _ in range(2):
                outf = engf.vjp(A_bm, xr, yr, sr, dxt, dyt, path="per_instance_dense")
                torch.cuda.synchronize()
            assert engf.plan()["last_fast"] == fv, (tag, fv, engf.plan()["last_fast"])
            assert ((outf[2].cpu().numpy() & 3) == 0).all(), (tag, fv)
            assert _rel(outf[0].cpu().numpy().T, want.T) < 1e-5 and _rel(outf[1].cpu().numpy()[:n].T, g["dc"]) < 1e-5, (tag, "forced first tile", fv)
            if fv in first_tiles(plan["brt_variant"]):
                assert all(torch.equal(a_, b_) for a_, b_ in zip(outf[:3], single)), (tag, "forced first tile", fv, "not bit-identical to the single tile")
    return plan


@pytest.mark.parametrize("family", pk.all_families())
def test_parity_at_plan_edges(family, monkeypatch):
    shapes, _, _ = discovery()
    vals = shapes.get(family, [])
    for v in vals:
        parity_at(family, v, monkeypatch)
    print(f"\n{family}: parity at {len(vals)} edge shapes {vals}")


def test_backward_rt_variant4_as_a_forced_first_tile(monkeypatch):
    """k_backward_rt variant 4 {7, 7, 7, 16} is the worst-case tile only for m < n templates (plan_kit.LEDGER_FAMILIES: no unique solution to compare);
    its code is checked against the oracle as the first tile of the two-tile plan forced on a variant-6 shape."""
    _, seen, _ = discovery()
    cands = sorted((pk.shape_of(fam, v)[0], fam, v) for fam, v, p in seen.values()
                   if p["brt_variant"] == 6 and p["two_tile"] and fam in pk.FAMILIES and fam.startswith(("zl_", "soc_", "mixed_")))
    assert cands, "no variant-6 shape among the plain families"
    _, fam, v = cands[0]
    plan = parity_at(fam, v, monkeypatch, force=(4,))
    print(f"\nk_backward_rt v4 forced as the first tile at {fam} v={v} (worst-case tile v{plan['brt_variant']})")


# --------------------------------------------------------------------------------------------------------- the rows of the shared-A kernels' lists
SA_V = {16: 3, 32: 20, 64: 40}          # sp_RP -> dense rows of the shared family (the edges 16 | 17, 32 | 33, 64 | 65 are swept above)
SA_B = 5


def sa_rows_at(RP, fam, monkeypatch, seed=0):
    """{ledger entry: where} of every k_sa_fwd / k_sa_lsqr row the shared template of SA_V[RP] dense rows and cone set `fam` reaches.  Every call is compared
    with the oracle as the existing test of its path does, at that test's tolerance:
      * forward and LSQR adjoint as parity_at (statuses equal, x / y / s within 1e-6; gradients within 1e-5 of the oracle's LSQR mode under TIGHT_LSQR);
      * LSMR as test_gpu_lsqr_mode.py (within 1e-6 of the oracle's LSMR mode under TIGHT_LSQR);
      * the forward derivative as test_gpu_jvp.py (the transpose identity against the adjoint kernel of the same path, to 1e-6 (1 + |lhs| + |rhs|));
    and the row ce_get_plan reports behind it must be the one named HERE from the cones and the switches.  Results are cached: the ledger and the parity test share them."""
    if ("sa", RP, fam) in _CACHE:
        return _CACHE[("sa", RP, fam)]
    from oracle import oracle
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings
    v, B, dev = SA_V[RP], SA_B, torch.device("cuda", 0)
    n, m, cones, pat, _, A, b, c, _, ref = _oracle_data(fam, v, B, seed, False)
    psd, tri = int("s" in cones), int("ep" in cones)
    tpl = P.dense_template(n, cones, pattern=pat)
    eng = ConeEngine(tpl.indices, tpl.indptr, n, m, cones, dev)
    plan = eng.plan()
    tag = f"{fam} v={v} n={n} m={m}"
    assert plan["sp_RP"] == RP and plan["last_sa_fwd"] == -1 and plan["last_sa_lsqr"] == -1, (tag, plan)
    fwd_rows = [sa_fwd_name(*r[1:]) for r in pk.variant_rows("CE_SA_FWD_VARIANTS")]
    lsqr_rows = [sa_lsqr_name(*r[1:]) for r in pk.variant_rows("CE_SA_LSQR_VARIANTS")]
    reached = {}

    def ran(field, rows, want, sw):
        got = rows[eng.plan()[field]] if eng.plan()[field] >= 0 else None
        assert got == want, (tag, sw, "ran", got, "expected", want)
        reached.setdefault(want, f"{tag} {sw or ''}".rstrip())

    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    A_bm = eng.to_batch_major(torch.from_numpy(A_eval).to(dev)); q_t = torch.from_numpy(q_eval).to(dev)
    with monkeypatch.context() as mp:
        mp.setenv("CE_CONST_A", "1")
        # ---- forward: 256 threads by default at these sizes; 512 threads (templates without a PSD block) with the index arrays in LDS, and without
        fwd_calls = [({}, (RP, 256, 0, 1))]
        if not psd:
            fwd_calls += [({"CE_SA_NT": "512"}, (RP, 512, 1, tri)), ({"CE_SA_NT": "512", "CE_SA_CIDX": "0"}, (RP, 512, 0, 1))]
        for sw, row in fwd_calls:
            with mp.context() as mq:
                for e, val in sw.items():
                    mq.setenv(e, val)
                x, y, s, _, status, _ = eng.solve(A_bm, q_t, make_settings(dict(eps=EPS, max_iters=MAX_IT, acceleration_lookback=0)))
                torch.cuda.synchronize()
            assert eng.last_const_a_kernel == "k_sa_fwd", (tag, sw)
            assert (status.cpu().numpy() == ref["status"]).all(), (tag, sw, status.cpu().numpy())
            for nm, got, want in (("x", x, ref["x"]), ("y", y, ref["y"]), ("s", s, ref["s"])):
                print(f"  {tag} {sw} forward {nm}: {_rel(got.cpu().numpy(), want):.2e}")
                assert _rel(got.cpu().numpy(), want) < 1e-6, (tag, sw, nm, _rel(got.cpu().numpy(), want))
            ran("last_sa_fwd", fwd_rows, sa_fwd_name(*row), sw)
        # ---- adjoints at the oracle's point
        rng = np.random.default_rng(seed + 7)
        dx = rng.standard_normal((B, n)); dy = rng.standard_normal((B, m))
        xr, yr, sr, dxt, dyt = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (ref["x"], ref["y"], ref["s"], dx, dy))
        rule = dict(lsqr_atol=TIGHT_LSQR[0], lsqr_btol=TIGHT_LSQR[1], lsqr_iter_lim=TIGHT_LSQR[2])
        g = oracle.adjoint_batch(A, b, c, cones, ref["x"], ref["y"], ref["s"], dx, dy, mode="lsqr", **rule)
        gm = oracle.adjoint_batch(A, b, c, cones, ref["x"], ref["y"], ref["s"], dx, dy, mode="lsmr", **rule)
        want, want_m = _boundary(tpl, g, n), _boundary(tpl, gm, n)
        # the leanest instantiation that has the cones' code: plain, PSD without triples (not for per-instance values, RP = 0), general
        lean = lambda rp: (0, 0) if not (psd or tri) else (1, 0) if (rp > 0 and not tri) else (1, 1)
        adj_calls = [("const_a", {}, (RP,) + lean(RP)), ("per_instance_lsqr", {}, (0,) + lean(0))]
        if not tri:
            adj_calls.append(("const_a", {"CE_SA_LSQR_SPEC": "0"}, (RP, 1, 1)))          # (the general kernel on request)
        kept = {}
        for path, sw, row in adj_calls:
            with mp.context() as mq:
                for e, val in sw.items():
                    mq.setenv(e, val)
                dA, dq, adj = eng.vjp(A_bm, xr, yr, sr, dxt, dyt, path=path, lsqr=TIGHT_LSQR, q_eval=q_t)
                torch.cuda.synchronize()
            dAn, dqn = dA.cpu().numpy(), dq.cpu().numpy()
            print(f"  {tag} {path} {sw} adjoint: dA {_rel(dAn.T, want.T):.2e} dc {_rel(dqn[:n].T, g['dc']):.2e}")
            assert (adj.cpu().numpy() == 0).all(), (tag, path, sw, adj)
            assert _rel(dAn.T, want.T) < 1e-5, (tag, path, sw, "dA", _rel(dAn.T, want.T))
            assert _rel(dqn[:n].T, g["dc"]) < 1e-5, (tag, path, sw, "dc")
            assert np.abs(dqn[n]).max() == 0
            ran("last_sa_lsqr", lsqr_rows, sa_lsqr_name(*row, 0, 0), f"{path} {sw or ''}")
            kept.setdefault(path, (dA, dq))
        if not psd and not tri:          # plain cones: ce_vjp is the search-free elimination and, behind it, the fixed grid of the plain RP = 0 row over the re-solve list
            assert plan["ns_variant"] >= 0, (tag, plan)
            dA, dq, adj = eng.vjp(A_bm, xr, yr, sr, dxt, dyt, path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t)
            torch.cuda.synchronize()
            assert ((adj.cpu().numpy() & 3) == 0).all(), (tag, "re-solve", adj)
            assert _rel(dA.cpu().numpy().T, want.T) < 1e-5 and _rel(dq.cpu().numpy()[:n].T, g["dc"]) < 1e-5, (tag, "re-solve")
            ran("last_sa_lsqr", lsqr_rows, sa_lsqr_name(0, 0, 0, 0, 0), "per_instance (re-solve list)")
        for path, row in (("const_a", (RP, 1, 1, 1, 0)), ("per_instance_lsqr", (0, 1, 1, 1, 0))):
            dA, dq, adj = eng.vjp(A_bm, xr, yr, sr, dxt, dyt, path=path, lsqr=TIGHT_LSQR + ("full", "lsmr"), q_eval=q_t)
            torch.cuda.synchronize()
            dAn, dqn = dA.cpu().numpy(), dq.cpu().numpy()
            print(f"  {tag} {path} LSMR: dA {np.abs(dAn - want_m).max() / (1 + np.abs(want_m).max()):.2e}")
            assert (adj.cpu().numpy() == 0).all(), (tag, path, "lsmr", adj)
            assert np.abs(dAn - want_m).max() < 1e-6 * (1 + np.abs(want_m).max()), (tag, path, "lsmr dA")
            assert np.abs(dqn[:n] - gm["dc"].T).max() < 1e-6 * (1 + np.abs(gm["dc"]).max()), (tag, path, "lsmr dc")
            ran("last_sa_lsqr", lsqr_rows, sa_lsqr_name(*row), f"{path} lsmr")
        # ---- forward derivative: plain cones, or the general kernel.  A shared A has no tangent (b and c alone); per-instance values have one
        for path, vpath, rp, with_A in (("const_a", "const_a", RP, False), ("per_instance", "per_instance_lsqr", 0, True)):
            trng = np.random.default_rng(seed + 9)
            tA = trng.standard_normal((B, m, n)) * pat if with_A else np.zeros((B, m, n))
            tA_eval, tq_eval = tpl.values_from_dense(tA, trng.standard_normal((B, m)), trng.standard_normal((B, n)))
            tA_bm = torch.from_numpy(tA_eval).to(dev).t().contiguous(); tq = torch.from_numpy(tq_eval).to(dev)
            jx, jy, _, st = eng.jvp(A_bm, xr, yr, sr, tA_bm, tq, path=path, lsqr=TIGHT_LSQR, q_eval=q_t)
            torch.cuda.synchronize()
            assert (st.cpu().numpy() == 0).all(), (tag, path, "jvp", st)
            dA, dq = kept[vpath]
            lhs = ((dxt * jx).sum(dim=1) + (dyt * jy).sum(dim=1)).cpu().numpy()
            rhs = ((dA.t() * tA_bm).sum(dim=1) + (dq * tq).sum(dim=0)).cpu().numpy()
            print(f"  {tag} {path} forward derivative: transpose identity {(np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))).max():.2e}")
            assert (np.abs(lhs - rhs) < 1e-6 * (1 + np.abs(lhs) + np.abs(rhs))).all(), (tag, path, lhs, rhs)
            assert np.abs(lhs).max() > 1e-3
            plain = not psd and not tri
            ran("last_sa_lsqr", lsqr_rows, sa_lsqr_name(rp, int(not plain), int(not plain), 0, 1), f"{path} jvp")
    _CACHE[("sa", RP, fam)] = reached
    return reached


@pytest.mark.parametrize("fam", list(pk.SHARED_CONE_SETS))
@pytest.mark.parametrize("RP", list(SA_V))
def test_shared_a_kernel_rows(RP, fam, monkeypatch):
    reached = sa_rows_at(RP, fam, monkeypatch)
    print(f"\n{fam} sp_RP={RP}: {len(reached)} rows")
    for var, where in reached.items():
        print(f"  {var:50s} {where}")

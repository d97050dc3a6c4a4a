"""libcone_engine.so and the g++ build of csrc/ce_plan.h plan alike: at the edge shapes plan_kit's discovery keeps (the last shape before and the first after
each plan change under the default switches, per family, the ledger-only families included: where a comparison in one build of the header could fall the other way
in the other, and the smallest such shapes), under every create-time switch, what ce_get_plan / ce_get_launch_info report of a created engine equals the host plan
field for field.  Edges that exist only under a switch are not discovered here; tests/test_plan_host.py holds every value under every switch to the recorded table.
Engines are created only; no kernel is launched."""
import pytest
import torch

import plan_kit as pk
from cvxpylayers_amd import _lib, problems as P

pytestmark = pytest.mark.gpu

# ce_get_plan's create-time fields (last_fast, last_sa_fwd, last_sa_lsqr are call history: -1 on a fresh engine) and ce_get_launch_info's
PLAN_KEYS = ("fwd_mode", "f2_variant", "rt_variant", "wl", "aa_ok", "gen_blocked_f", "qp_native", "bwd_mode", "brt_variant", "two_tile", "ns_variant", "gen_blocked_b", "sp_r", "sp_RP")
INFO_KEYS = {"fwd_lds_bytes": "fwd_lds", "bwd_lds_bytes": "bwd_lds", "fwd_mode": "fwd_mode", "bwd_mode": "bwd_mode"}


def _engine_plan(fam, v):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    n, cones, pat, pstruct = pk.shape_of(fam, v)
    tpl = P.dense_template(n, cones, pattern=pat)
    try:
        eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0), p_structure=pstruct)
    except (NotImplementedError, _lib.EngineError):
        return None
    out = (eng.plan(), dict(eng._launch_info), eng.qp_native)
    del eng
    return out


def _edge_shapes():
    """{family: values}: both sides of every plan change of the family's sweep (host plan, default switches), refused shapes dropped"""
    return {fam: pk.edge_shapes(pk.find_edges(lambda v, fam=fam: pk.host_plan_of(fam, v), pk.family_values(fam), fields=pk.fields_for(fam))) for fam in pk.all_families(ledger=True)}


def test_library_and_host_build_plan_alike(monkeypatch):
    for e in pk.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)
    shapes = _edge_shapes()
    assert all(shapes[fam] for fam in shapes), shapes
    compared = 0
    for sw in pk.SWITCHES:
        with monkeypatch.context() as mp:
            for e, val in sw.items():
                mp.setenv(e, val)
            for fam, vals in shapes.items():
                for v in vals:
                    host, got = pk.host_plan_of(fam, v), _engine_plan(fam, v)
                    assert (host is None) == (got is None), (fam, v, sw, host, got)
                    if host is None:
                        continue
                    plan, info, qp_native = got
                    assert {k: plan[k] for k in PLAN_KEYS} == {k: host[k] for k in PLAN_KEYS}, (fam, v, sw)
                    assert all(plan[k] == -1 for k in ("last_fast", "last_sa_fwd", "last_sa_lsqr")), (fam, v, sw, plan)
                    assert {k: info[k] for k in INFO_KEYS} == {k: host[h] for k, h in INFO_KEYS.items()}, (fam, v, sw, info, host)
                    assert qp_native == bool(host["qp_native"]), (fam, v, sw)
                    compared += 1
    print(f"\n{compared} engines compared with the host plan at {sum(len(v) for v in shapes.values())} edge shapes under {len(pk.SWITCHES)} switch sets")

"""CPU: plan_kit's edge finding and deduplication on synthetic plan functions (the GPU side, tests/test_gpu_plan_edges.py, points them at ce_get_plan)."""
import plan_kit as pk


def synthetic_plan(v, **over):
    """a step function of v: f2 variants by thresholds (an exact-fill edge at 32 | 33), k_forward_rt above 60, refused from 90"""
    if v >= 90:
        return None
    p = {f: 0 for f in pk.EDGE_FIELDS}
    p.update(sp_r=v, last_fast=-1)                    # (not edge fields: change with every v)
    if v <= 32:
        p.update(fwd_mode=4, f2_variant=0 if v <= 14 else 1)
    elif v <= 60:
        p.update(fwd_mode=4, f2_variant=2)
    else:
        p.update(fwd_mode=3, f2_variant=-1, rt_variant=0)
    p.update(over)
    return p


def test_edges_are_the_last_value_before_and_the_first_after_each_change():
    edges = pk.find_edges(synthetic_plan, range(1, 100))
    assert [(e[0], e[2]) for e in edges] == [(14, 15), (32, 33), (60, 61), (89, 90)]
    assert edges[-1][3] is None and edges[-1][1]["rt_variant"] == 0
    assert pk.edge_shapes(edges) == [14, 15, 32, 33, 60, 61, 89]           # the refused side is not a shape to test


def test_steps_of_one_find_an_exact_fill_edge_that_coarser_steps_miss():
    assert (32, 33) in [(e[0], e[2]) for e in pk.find_edges(synthetic_plan, range(1, 100))]
    assert (32, 33) not in [(e[0], e[2]) for e in pk.find_edges(synthetic_plan, range(1, 100, 4))]


def test_fields_outside_the_key_do_not_make_edges():
    assert pk.find_edges(lambda v: synthetic_plan(20, sp_r=v, last_fast=v % 3), range(50)) == []
    assert len(pk.find_edges(lambda v: synthetic_plan(20, sp_RP=16 if v <= 16 else 32), range(1, 40))) == 1


def test_dedupe_keeps_one_edge_per_pair_of_plans():
    # the same transition met in two sweeps (and twice in one: up, down, up) is kept once, the first time
    flip = lambda v: synthetic_plan(20 if (v // 10) % 2 == 0 else 40)
    edges = pk.find_edges(flip, range(0, 40)) + pk.find_edges(synthetic_plan, range(1, 100))
    assert [(e[0], e[2]) for e in edges][:3] == [(9, 10), (19, 20), (29, 30)]
    d = pk.dedupe(edges)
    assert [(e[0], e[2]) for e in d] == [(9, 10), (19, 20), (14, 15), (60, 61), (89, 90)]
    # (32 -> 33 is f2 1 -> 2, the pair the flip met first at 9 -> 10; 14 -> 15 is 0 -> 1, new)
    assert len(pk.dedupe(d)) == len(d)


def test_families_are_valid_templates():
    from cvxpylayers_amd import problems as P
    for fam in pk.all_families(ledger=True):
        vals = list(pk.family_values(fam))
        for v in (vals[0], vals[len(vals) // 2], vals[-1]):
            n, cones, pat, pstruct = pk.shape_of(fam, v)
            m = P.cone_rows(cones)
            assert (m >= n or fam in pk.LEDGER_FAMILIES) and min(cones.get("l", 0), cones.get("z", 0)) >= 0, (fam, v, n, cones)
            tpl = P.dense_template(n, cones, pattern=pat)
            assert tpl.m == m and tpl.indptr[-1] == len(tpl.indices)
            if pstruct is not None:
                assert pstruct[1][-1] == len(pstruct[0]) == n * (n + 1) // 2

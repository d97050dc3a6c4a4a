"""The layout and the plan of the search-free elimination on templates with PSD blocks AND exponential / power triples, on the host (no GPU): csrc/ce_ns_layout.h
with both counts passed (the triples' two segments, then the blocks' five, no segment of its own; bwd_ns_psd_tri_lds_bytes_of) and csrc/ce_plan.h
psd_tri_ns_variant / psd_tri_ns_lds, compiled with g++ (psd_tri_ns_kit.host_lib, in the manner of psd_ns_kit.host_lib).  The mixed layout's segments are disjoint
and in order and equal a restatement of the kernel's pointer-bumping carve; the plan rows and footprints are pinned; the templates the mode does not serve get no
row; a mixed template leaves the four older variants at -1; the four older footprint functions return what they returned before the mode."""
import ctypes as C
import os

import pytest

import psd_ns_kit as PK
import psd_tri_ns_kit as K
import tri_ns_kit as TK
from cvxpylayers_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DBL, N_UNION, N_INT, N_TOP = 11, 6, 13, 7          # the order of h_layout_mixed: doubles, U and its five members, ints, Wt, lamt and the five PSD segments

# (n, cones) -> (row of CE_NS_VARIANTS, footprint in bytes), from ns_layout with both counts passed
EXTRA_PLAN = {
    "edge_108": ((108, {"z": 4, "l": 10, "q": [5], "s": [4], "ep": 2}), (2, 49096)),
    "edge_108_footprint": ((108, {"z": 4, "l": 60, "q": [5], "s": [16], "ep": 2}), (-1, 0)),
}
# (kit, shape, row) -> the plain, QP, TRI and PSD footprints of the four older functions, recorded from a g++ build of the header as it stood before the mixed mode
OLD_FOOTPRINTS = {
    ('psd', 'psd_small', 0): (4296, 4472, 4296, 5272),
    ('psd', 'psd_small', 1): (6344, 6520, 6344, 7320),
    ('psd', 'psd_small', 2): (10712, 10888, 10712, 12264),
    ('psd', 'psd_mixed', 0): (7824, 9120, 7824, 9680),
    ('psd', 'psd_mixed', 1): (9872, 11168, 9872, 11728),
    ('psd', 'psd_mixed', 2): (14240, 15536, 14240, 17120),
    ('psd', 'psd_only', 0): (6408, 7328, 6408, 8448),
    ('psd', 'psd_only', 1): (8456, 9376, 8456, 10496),
    ('psd', 'psd_only', 2): (12824, 13744, 12824, 15888),
    ('psd', 'lqr_like', 0): (13248, 18144, 13248, 17208),
    ('psd', 'lqr_like', 1): (15296, 20192, 15296, 19256),
    ('psd', 'lqr_like', 2): (19664, 24560, 19664, 25928),
    ('psd', 'row2_n80', 0): (66692, 118856, 66692, 73568),
    ('psd', 'row2_n80', 1): (68740, 120904, 68740, 75616),
    ('psd', 'row2_n80', 2): (73108, 125272, 73108, 84080),
    ('tri', 'exp_small', 0): (4800, 5160, 4992, 4800),
    ('tri', 'exp_small', 1): (6848, 7208, 7040, 6848),
    ('tri', 'exp_small', 2): (11216, 11576, 11408, 11216),
    ('tri', 'exp_pow_mixed', 0): (7584, 8880, 7968, 7584),
    ('tri', 'exp_pow_mixed', 1): (9632, 10928, 10016, 9632),
    ('tri', 'exp_pow_mixed', 2): (14000, 15296, 14384, 14000),
    ('tri', 'triples_only', 0): (5760, 6524, 6240, 5760),
    ('tri', 'triples_only', 1): (7808, 8572, 8288, 7808),
    ('tri', 'triples_only', 2): (12176, 12940, 12656, 12176),
    ('tri', 'E', 0): (37632, 50912, 39936, 37632),
    ('tri', 'E', 1): (39680, 52960, 41984, 39680),
    ('tri', 'E', 2): (44048, 57328, 46352, 44048),
    ('tri', 'row2_n80', 0): (87380, 139544, 88920, 87380),
    ('tri', 'row2_n80', 1): (88884, 141048, 90424, 88884),
    ('tri', 'row2_n80', 2): (93252, 145416, 94792, 93252),
}


@pytest.fixture(scope="module")
def host():
    return K.host_lib()


def _row(host, v):
    a, b = C.c_int(), C.c_int()
    host.h_row(v, C.byref(a), C.byref(b))
    return a.value, b.value


def _sizes(n, cones):
    """(n, m, nq, ntri, ns, maxs, psdrows) as the shim's functions take them"""
    s = cones.get("s", [])
    return n, K.m_of(cones), len(cones.get("q", [])), K.ntri(cones), len(s), max(s) if s else 0, K.psd_rows(cones)


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_mixed_segments_are_disjoint_in_order_and_equal_the_kernels_carve(host, shape, monkeypatch):
    """fails on a tree without the mode: bwd_ns_psd_tri_lds_bytes_of and CePlan::psd_tri_ns_variant do not exist, the shim does not compile"""
    for e in K.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)
    n, cones, _, _ = K.SHAPES[shape]
    sz = _sizes(n, cones)
    _, m, nq, ntri, ns, maxs, psdrows = sz
    plan = K.host_plan(n, cones)
    assert (plan["psd_tri_ns_variant"], plan["psd_tri_ns_lds"]) == K.PLAN[shape], plan
    assert plan["ns_variant"] == plan["qp_ns_variant"] == plan["tri_ns_variant"] == plan["psd_ns_variant"] == -1, plan          # the four older variants stay -1
    for v in range(host.h_rows()):
        ntile, nthr = _row(host, v)
        nwb = nthr // 64
        carve = (C.c_long * 8)(); lay = (C.c_long * 96)()
        host.h_carve_mixed(*sz, ntile, nthr, carve)
        k = host.h_layout_mixed(*sz, ntile, nthr, lay)
        assert k == N_DBL + N_UNION + N_INT + N_TOP
        seg = [(lay[2 * i], lay[2 * i + 1]) for i in range(k)]
        slack, total = lay[2 * k], lay[2 * k + 1]
        assert all(off >= 0 and ln >= 0 and off + ln <= total for off, ln in seg), (shape, v, seg, total)
        top = seg[-N_TOP:]
        assert [off for off, _ in top] == list(carve[:7]) and top[-1][0] + top[-1][1] == carve[7] == slack <= total <= carve[7] + 16, (shape, v, top, list(carve), total)
        assert [ln for _, ln in top] == [8 * 9 * ntri, 8 * 3 * ntri, 8 * ns * maxs * maxs, 8 * ns * maxs, 8 * psdrows, 8 * (2 * maxs * maxs + 2 * maxs + 8), 8 * 2 * nwb * maxs * maxs]
        assert all(off % 8 == 0 for off, _ in top)
        # in order: Wt, lamt, then psdU ... psdXW, each behind the one before, all behind the ints
        for (o0, l0), (o1, _) in zip(top, top[1:]):
            assert o0 + l0 <= o1, (shape, v, top)
        assert top[0][0] >= max(off + ln for off, ln in seg[N_DBL + N_UNION:N_DBL + N_UNION + N_INT])
        # disjoint: every segment but the five members of the union region (which lie inside U, the plain layout's declared phase aliases)
        u_off, u_len = seg[N_DBL]
        members = seg[N_DBL + 1:N_DBL + N_UNION]
        assert all(u_off <= off and off + ln <= u_off + u_len for off, ln in members), (shape, v)
        solid = sorted(seg[:N_DBL + 1] + seg[N_DBL + N_UNION:])
        for (o0, l0), (o1, _) in zip(solid, solid[1:]):
            assert o0 + l0 <= o1, (shape, v, (o0, l0), o1)
        fp = (C.c_long * 5)()
        host.h_footprints5(*sz, ntile, nthr, fp)
        assert fp[4] == total and total - fp[0] in (sum(ln for _, ln in top), sum(ln for _, ln in top) + 4), (shape, v)          # on top of the plain footprint (+ the rounding of the ints)
        assert fp[4] > fp[3] > fp[0] and fp[4] > fp[2] > fp[0]
        if v == plan["psd_tri_ns_variant"]:
            assert plan["psd_tri_ns_lds"] == total
        if v < plan["psd_tri_ns_variant"]:          # the rows in front of the chosen one do not hold the reduced system or exceed LDS
            assert 4 * ((n + 3) // 4) + 1 > 16 * ntile or total > 160 * 1024


def test_plan_rows_at_the_largest_n(host, monkeypatch):
    for e in K.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)
    for name, ((n, cones), (row, by)) in EXTRA_PLAN.items():
        plan = K.host_plan(n, cones)
        assert (plan["psd_tri_ns_variant"], plan["psd_tri_ns_lds"]) == (row, by), (name, plan)
    n, cones = EXTRA_PLAN["edge_108_footprint"][0]          # refused by the footprint, not by the tiles: row 2 holds 109 columns
    fp = (C.c_long * 5)()
    host.h_footprints5(*_sizes(n, cones), *_row(host, 2), fp)
    assert fp[4] > 160 * 1024 and 4 * ((n + 3) // 4) + 1 <= 16 * _row(host, 2)[0]


def test_templates_that_get_no_mixed_variant(host, monkeypatch):
    for e in K.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)
    mixed = K.SHAPES["mix_small"][:2]
    assert K.host_plan(*mixed)["psd_tri_ns_variant"] == 0
    assert K.host_plan(*PK.SHAPES["lqr_like"][:2])["psd_tri_ns_variant"] == -1                               # a pure PSD template: psd_ns_variant serves it
    assert K.host_plan(*PK.SHAPES["lqr_like"][:2])["psd_ns_variant"] == 0
    assert K.host_plan(*TK.SHAPES["exp_pow_mixed"][:2])["psd_tri_ns_variant"] == -1                          # a pure triple template: tri_ns_variant serves it
    assert K.host_plan(*TK.SHAPES["exp_pow_mixed"][:2])["tri_ns_variant"] == 0
    assert K.host_plan(12, {"z": 2, "l": 6, "q": [4, 5]})["psd_tri_ns_variant"] == -1                        # plain cones
    assert K.host_plan(12, {"z": 2, "l": 14, "q": [], "s": [3], "ep": 1}, nnz_p=1)["psd_tri_ns_variant"] == -1   # a quadratic objective
    assert K.host_plan(109, {"z": 4, "l": 10, "q": [5], "s": [4], "ep": 2})["psd_tri_ns_variant"] == -1       # n > 108
    monkeypatch.setenv("CE_BWD_NS", "0")
    assert K.host_plan(*mixed)["psd_tri_ns_variant"] == -1
    monkeypatch.delenv("CE_BWD_NS")
    monkeypatch.setenv("CE_FORCE_GENERIC", "1")
    assert K.host_plan(*mixed)["psd_tri_ns_variant"] == -1


def test_the_four_older_footprint_functions_return_what_they_returned(host):
    fp = (C.c_long * 5)()
    for (kit, name, v), want in OLD_FOOTPRINTS.items():
        n, cones = (PK.SHAPES if kit == "psd" else TK.SHAPES)[name][:2]
        host.h_footprints5(*_sizes(n, cones), *_row(host, v), fp)
        assert tuple(fp[:4]) == want, ((kit, name, v), tuple(fp[:4]), want)


def test_the_symbols_are_declared_bound_and_exported_and_the_objects_listed():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    for sym, sib in (("ce_jvp_psd_tri", "ce_jvp_psd"), ("ce_refine_psd_tri", "ce_refine_psd"), ("ce_vjp_psd_tri_many", "ce_vjp_psd_many"), ("ce_jvp_psd_tri_many", "ce_jvp_psd_many")):
        assert sym in _lib.SYMBOLS and hasattr(L, sym) and (sym + "(ce_handle h") in hdr, sym
        assert getattr(L, sym).argtypes == getattr(L, sib).argtypes, sym          # the arguments of the PSD sibling
    for sym in ("ce_psd_tri_ns_variant", "ce_psd_tri_ns_lds", "ce_vjp_psd_tri_many_variant", "ce_jvp_psd_tri_many_variant"):
        assert sym in _lib.SYMBOLS and (sym + "(ce_handle h);") in hdr, sym
    assert L.ce_psd_tri_ns_variant(None) == -1 and L.ce_psd_tri_ns_lds(None) == 0 and L.ce_vjp_psd_tri_many_variant(None) == -1 and L.ce_jvp_psd_tri_many_variant(None) == -1
    import re
    assert int(re.search(r"#define CE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == L.ce_abi_version() == _lib.ABI_VERSION
    from cvxpylayers_amd.interfaces.cone_engine import ConeEngine
    assert len(ConeEngine.PLAN_FIELDS) == 18 and hasattr(ConeEngine, "psd_tri_ns_plan")
    csrc = os.path.dirname(_lib.SO_PATH)
    mk = open(os.path.join(csrc, "Makefile")).read()
    objs = mk.split("OBJS")[1].split("all:")[0]
    for unit, obj, n_inst in (("ce_tu_ns_psd_tri.hip", "$(OBJDIR)/ns_psd_tri.o", "true, REF, false, true, false, true>"),
                              ("ce_tu_ns_vjp_psd_tri_many.hip", "$(OBJDIR)/ns_vjp_psd_tri_many.o", "false, false, false, true, true, true>"),
                              ("ce_tu_ns_jvp_psd_tri_many.hip", "$(OBJDIR)/ns_jvp_psd_tri_many.o", "true, false, false, true, true, true>")):
        src = open(os.path.join(csrc, unit)).read()
        assert unit in mk and obj in objs and "CE_NS_VARIANTS(X)" in src and src.count(n_inst) == 2, unit          # every row, launch and attribute alike


def test_the_notices_no_longer_name_triples_as_a_reason():
    import warnings
    from cvxpylayers_amd.interfaces import solver_args as SA
    for key, call in (("psd_elimination", lambda: SA.psd_elimination_active("search_free", -1, True)),
                      ("psd_adjoint", lambda: SA.psd_many_active("psd_adjoint", True, -1, True)), ("psd_tangents", lambda: SA.psd_many_active("psd_tangents", True, -1, True))):
        SA._WARNED.discard(key + "_none")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert call() is False
        assert len(w) == 1 and "ignored on this template" in str(w[0].message) and "exponential" not in str(w[0].message), [str(x.message) for x in w]
    # a served mixed template (the caller passes psd_tri_ns_variant) is active and silent
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert SA.psd_elimination_active("search_free", 0, True) and SA.psd_many_active("psd_adjoint", True, 0, True) and SA.psd_many_active("psd_tangents", True, 0, True)
    assert not w

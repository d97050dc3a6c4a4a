"""The PSD mode of k_backward_ns' LDS layout (cvxpylayers_amd/csrc/ce_ns_layout.h: per block U and Lambda, per rotated row B, the Jacobi scratch and the rotation's
per-wave pairs behind the index arrays) and the plan that is made on it (csrc/ce_plan.h psd_ns_variant / psd_ns_lds), compiled with g++ in the manner of
test_tri_ns_layout_host.py (the shim lives in psd_ns_kit.py: test_gpu_psd_jvp.py asks it for the row the engine must report).  For the five shapes of
psd_ns_kit.SHAPES the segments lie inside the footprint, equal a restatement of the kernel's pointer-bumping carve and are disjoint except for the declared
aliases -- the members of the union region, which is the plain layout's own; no PSD segment aliases anything --, the plain / QP / TRI footprints are what they were,
and the templates the mode does not serve get no row."""
import ctypes as C

import pytest

import psd_ns_kit as K
from cvxpylayers_amd import _lib

N_DBL, N_UNION, N_INT, N_PSD = 11, 6, 13, 5          # the order of h_layout_psd: doubles, U and its five members, ints, the PSD segments


@pytest.fixture(scope="module")
def host():
    return K.host_lib()


def _row(host, v):
    a, b = C.c_int(), C.c_int()
    host.h_row(v, C.byref(a), C.byref(b))
    return a.value, b.value


def _sizes(cones):
    s = cones.get("s", [])
    return len(cones.get("q", [])), len(s), max(s), sum(k * (k + 1) // 2 for k in s)


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_psd_segments_lie_inside_the_footprint_and_alias_nothing(host, shape, monkeypatch):
    for e in K.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)
    n, cones, _, _ = K.SHAPES[shape]
    m = K.m_of(cones)
    nq, ns, maxs, psdrows = _sizes(cones)
    plan = K.host_plan(n, cones)
    assert plan["psd_ns_variant"] >= 0 and plan["ns_variant"] == -1 and plan["qp_ns_variant"] == -1 and plan["tri_ns_variant"] == -1 and plan["bwd_mode"] == 3, plan
    for v in range(host.h_rows()):
        ntile, nthr = _row(host, v)
        nwb = nthr // 64
        carve = (C.c_long * 6)(); lay = (C.c_long * 80)()
        host.h_carve_psd(n, m, nq, ns, maxs, psdrows, ntile, nthr, carve)
        k = host.h_layout_psd(n, m, nq, ns, maxs, psdrows, ntile, nthr, lay)
        assert k == N_DBL + N_UNION + N_INT + N_PSD
        seg = [(lay[2 * i], lay[2 * i + 1]) for i in range(k)]
        slack, total = lay[2 * k], lay[2 * k + 1]
        assert all(off >= 0 and ln >= 0 and off + ln <= total for off, ln in seg), (shape, v, seg, total)
        psd = seg[-N_PSD:]
        assert [off for off, _ in psd] == list(carve[:5]) and psd[-1][0] + psd[-1][1] == carve[5] == slack <= total <= carve[5] + 16, (shape, v, psd, list(carve), total)
        assert [ln for _, ln in psd] == [8 * ns * maxs * maxs, 8 * ns * maxs, 8 * psdrows, 8 * (2 * maxs * maxs + 2 * maxs + 8), 8 * 2 * nwb * maxs * maxs]
        assert all(off % 8 == 0 for off, _ in psd)
        # disjoint: every segment but the five members of the union region (which lie inside U, the plain layout's declared phase aliases)
        u_off, u_len = seg[N_DBL]
        members = seg[N_DBL + 1:N_DBL + N_UNION]
        assert all(u_off <= off and off + ln <= u_off + u_len for off, ln in members), (shape, v)
        solid = sorted(seg[:N_DBL + 1] + seg[N_DBL + N_UNION:])
        for (o0, l0), (o1, _) in zip(solid, solid[1:]):
            assert o0 + l0 <= o1, (shape, v, (o0, l0), o1)
        fp = (C.c_long * 5)()
        host.h_footprints(n, m, nq, 0, ns, maxs, psdrows, ntile, nthr, fp)
        assert fp[3] == total and total - fp[0] in (sum(ln for _, ln in psd), sum(ln for _, ln in psd) + 4), (shape, v)          # on top of the plain footprint (+ the rounding of the ints)
        if v == plan["psd_ns_variant"]:
            assert plan["psd_ns_lds"] == total
        if v < plan["psd_ns_variant"]:          # the rows in front of the chosen one do not hold the reduced system or exceed LDS
            assert 4 * ((n + 3) // 4) + 1 > 16 * ntile or total > 160 * 1024


def test_plain_qp_and_tri_footprints_are_unchanged(host):
    """the quoted footprints of test_ns_layout_host.py / test_tri_ns_layout_host.py through the new signature; none of the three modes has a byte of the PSD segments"""
    fp = (C.c_long * 5)()
    host.h_footprints(50, 100, 0, 0, 2, 6, 31, 4, 256, fp)
    assert (fp[0], fp[1], fp[2]) == (52496, 73096, 52496) and fp[4] == 0 and fp[3] > fp[0]
    for name, (n, cones, _, _) in K.SHAPES.items():
        m = K.m_of(cones)
        nq, ns, maxs, psdrows = _sizes(cones)
        for v in range(host.h_rows()):
            host.h_footprints(n, m, nq, 3, ns, maxs, psdrows, *_row(host, v), fp)
            assert fp[4] == 0 and fp[2] - fp[0] in (96 * 3, 96 * 3 + 4) and fp[1] > fp[0] and fp[3] > fp[0], (name, v, list(fp))
    # (n, m, nq, row) at three sizes, one per row of CE_NS_VARIANTS: the plain, QP and TRI (3 triples) footprints of the header as it stood before the PSD mode,
    # written down from a g++ build of that header
    for (n, m, nq, v), want in {(4, 7, 0, 0): (4296, 4472, 4584), (24, 41, 0, 1): (16472, 21368, 16760), (80, 88, 2, 2): (73868, 126032, 74160)}.items():
        host.h_footprints(n, m, nq, 3, 1, 2, 3, *_row(host, v), fp)
        assert tuple(fp[:3]) == want, ((n, m, nq, v), tuple(fp[:3]))


def test_templates_that_get_no_psd_variant(host, monkeypatch):
    for e in K.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)
    lqr = K.SHAPES["lqr_like"][1]
    assert K.host_plan(24, lqr)["psd_ns_variant"] == 0          # (25 columns: the two tiles of row 0)
    assert K.host_plan(12, {"z": 2, "l": 6, "q": [4, 5]})["psd_ns_variant"] == -1                          # plain cones: ns_variant serves them
    assert K.host_plan(6, {"z": 1, "l": 2, "s": [2], "ep": 1})["psd_ns_variant"] == -1                     # a block beside a triple
    assert K.host_plan(6, {"z": 1, "l": 2, "s": [2], "p": [0.3]})["psd_ns_variant"] == -1
    assert K.host_plan(12, {"z": 2, "l": 14, "q": [], "s": [3]}, nnz_p=1)["psd_ns_variant"] == -1           # a quadratic objective
    assert K.host_plan(112, {"z": 2, "l": 120, "q": [], "s": [3]})["psd_ns_variant"] == -1                 # n > 108
    assert K.host_plan(108, {"z": 2, "l": 120, "q": [], "s": [3]})["psd_ns_variant"] == 2
    monkeypatch.setenv("CE_BWD_NS", "0")
    assert K.host_plan(24, lqr)["psd_ns_variant"] == -1
    monkeypatch.delenv("CE_BWD_NS")
    monkeypatch.setenv("CE_FORCE_GENERIC", "1")
    assert K.host_plan(24, lqr)["psd_ns_variant"] == -1


def test_other_plan_fields_do_not_move(host, monkeypatch):
    """ns_variant / qp_ns_variant / tri_ns_variant and their footprints on templates of their own kinds, beside a psd_ns_variant of -1"""
    for e in K.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)
    p = K.host_plan(12, {"z": 2, "l": 6, "q": [4, 5]})
    assert (p["ns_variant"], p["qp_ns_variant"], p["tri_ns_variant"], p["psd_ns_variant"], p["psd_ns_lds"]) == (0, -1, -1, -1, 0) and p["ns_lds"] > 0
    p = K.host_plan(12, {"z": 2, "l": 6, "q": [4], "ep": 2, "p": [0.3, -0.6]})
    assert (p["ns_variant"], p["tri_ns_variant"], p["psd_ns_variant"]) == (-1, 0, -1) and p["tri_ns_lds"] > 0
    p = K.host_plan(6, {"z": 2, "l": 4, "q": []}, nnz_p=1)
    assert (p["ns_variant"], p["qp_ns_variant"], p["psd_ns_variant"]) == (-1, 0, -1) and p["qp_ns_lds"] > 0


def test_the_symbols_are_declared_bound_and_exported():
    import os
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cone_engine.h")).read()
    for sym in ("ce_jvp_psd", "ce_refine_psd", "ce_psd_ns_variant", "ce_psd_ns_lds"):
        assert sym in _lib.SYMBOLS and hasattr(L, sym) and (sym + "(ce_handle h") in hdr, sym
    assert L.ce_psd_ns_variant(None) == -1 and L.ce_psd_ns_lds(None) == 0
    assert L.ce_jvp_psd.argtypes == L.ce_jvp.argtypes and L.ce_refine_psd.argtypes == L.ce_refine.argtypes
    from cvxpylayers_amd.interfaces.cone_engine import ConeEngine
    assert ConeEngine.PLAN_FIELDS[-1] == "tri_ns_variant" and len(ConeEngine.PLAN_FIELDS) == 18 and hasattr(ConeEngine, "psd_ns_plan")
    mk = open(os.path.join(os.path.dirname(_lib.SO_PATH), "Makefile")).read()
    assert "ce_tu_ns_psd.hip" in mk and "$(OBJDIR)/ns_psd.o" in mk.split("OBJS")[1].split("all:")[0]

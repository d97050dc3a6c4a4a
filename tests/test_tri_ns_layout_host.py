"""The TRI mode of k_backward_ns' LDS layout (cvxpylayers_amd/csrc/ce_ns_layout.h: the eigenvectors and eigenvalues of the exponential / power triples behind the
index arrays) and the plan that is made on it (csrc/ce_plan.h tri_ns_variant / tri_ns_lds), compiled with g++ in the manner of test_ns_layout_host.py: for the
five shapes of tri_ns_kit.SHAPES the layout's segments equal a restatement of the kernel's pointer-bumping carve, the plan picks the expected row of
CE_NS_VARIANTS and leaves ns_variant / qp_ns_variant alone, and the plain and QP footprints are what they were."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tri_ns_kit as K
from cvxpylayers_amd import _lib, problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = r'''
#include <cstdio>
#include "ce_plan.h"
extern "C" {
// the kernel's carve (ce_backward_ns.h, TRI), restated with integer offsets: doubles from sm, then ints from (int *)sm, then the triples' doubles.
// out: first byte of Wt, of lamt, end of the carve
void h_carve_tri(int n, int m, int nq, int ntri, int NTILE, int NTHR, long *out) {
    const int NWB = NTHR / 64, nqs = nq > 0 ? nq : 1, npad = n + (n & 1), KWMAX = bwd_ns_kwmax(m), lda = n;
    long p = 0;
    p += (long)m * lda; p += p & 1;
    p += m; p += m; p += npad; p += npad; p += npad; p += 5 * nqs; p += KWMAX; p += KWMAX; p += NWB * 8; p += nqs;
    p += p & 1;
    p += bwd_ns_union_doubles(n, m, nqs, NTILE);
    long ip = 2 * p;
    ip += m; ip += m; ip += nqs; ip += nqs; ip += nqs; ip += n; ip += n; ip += n; ip += n; ip += KWMAX; ip += KWMAX; ip += NWB + 1; ip += 8;
    ip += ip & 1;
    out[0] = 4 * ip; out[1] = 4 * ip + 8L * 9 * ntri; out[2] = 4 * ip + 8L * 12 * ntri;
}
// out: first byte and byte count of Wt and lamt, first byte of slack, the footprint; the plain and QP footprints behind them
void h_layout_tri(int n, int m, int nq, int ntri, int NTILE, int NTHR, long *out) {
    const NsLayout L = ns_layout(n, m, nq, NTILE, NTHR, false, ntri);
    out[0] = 8L * L.Wt.off; out[1] = 8L * L.Wt.len; out[2] = 8L * L.lamt.off; out[3] = 8L * L.lamt.len; out[4] = 4L * L.slack.off; out[5] = (long)L.bytes;
    out[6] = (long)bwd_ns_tri_lds_bytes_of(n, m, nq, ntri, NTILE, NTHR); out[7] = (long)bwd_ns_lds_bytes_of(n, m, nq, NTILE, NTHR); out[8] = (long)bwd_ns_qp_lds_bytes_of(n, m, nq, NTILE, NTHR);
    const NsLayout L0 = ns_layout(n, m, nq, NTILE, NTHR, false), LQ = ns_layout(n, m, nq, NTILE, NTHR, true);
    out[9] = L0.Wt.len + L0.lamt.len + LQ.Wt.len + LQ.lamt.len; out[10] = (long)L0.bytes; out[11] = (long)LQ.bytes;
}
void h_row(int v, int *ntile, int *nthr) { *ntile = NS_ROWS[v].NTILE; *nthr = NS_ROWS[v].NTHR; }
int h_rows() { return (int)std::size(NS_ROWS); }
// out: ns_variant, qp_ns_variant, tri_ns_variant, tri_ns_lds, bwd_mode
int h_plan_tri(const ce_template *tpl, long *out) {
    DevT T{}; std::vector<int> qoff, soff; CePlan P;
    plan_sizes(tpl, T, qoff, soff);
    const int rc = plan_engine(tpl, T, tpl->nnz_p, read_plan_env(), P);
    if (rc) return rc;
    out[0] = P.ns_variant; out[1] = P.qp_ns_variant; out[2] = P.tri_ns_variant; out[3] = (long)P.tri_ns_lds; out[4] = P.bwd_mode;
    return 0;
}
}
'''
PLAN_ENV = ("CE_FWD", "CE_FORCE_GENERIC", "CE_BWD_NS", "CE_GEN_BLOCKED", "CE_WL", "CE_F2_NEUMANN", "CE_BWD_TWO_TILE", "CE_BWD_FAST_VARIANT")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("tri_ns_layout")
    (d / "host.cpp").write_text(SRC)
    so = str(d / "libtri_ns_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__host__=", "-D__device__=", "-shared", "-fPIC", "-I", os.path.join(ROOT, "cvxpylayers_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", so, str(d / "host.cpp")])
    L = C.CDLL(so)
    L.h_carve_tri.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_long)]; L.h_carve_tri.restype = None
    L.h_layout_tri.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_long)]; L.h_layout_tri.restype = None
    L.h_row.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.h_plan_tri.argtypes = [C.POINTER(_lib.CeTemplate), C.POINTER(C.c_long)]
    return L


def _template(n, cones, nnz_p=0):
    tpl = P.dense_template(n, cones)
    keep = [np.ascontiguousarray(tpl.indices, dtype=np.int32), np.ascontiguousarray(tpl.indptr, dtype=np.int32), np.ascontiguousarray(cones.get("q", []), dtype=np.int32),
            np.ascontiguousarray(cones.get("s", []), dtype=np.int32), np.ascontiguousarray(cones.get("p", []), dtype=np.float64)]
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))          # noqa: E731
    t = _lib.CeTemplate()
    t.n, t.m, t.nnz_aug, t.indices, t.indptr = int(tpl.n), int(tpl.m), int(keep[1][-1]), ip(keep[0]), ip(keep[1])
    t.z, t.l, t.nq, t.q, t.ns, t.s = int(cones.get("z", 0)), int(cones.get("l", 0)), len(keep[2]), ip(keep[2]), len(keep[3]), ip(keep[3])
    t.nep, t.np, t.p = int(cones.get("ep", 0)), len(keep[4]), keep[4].ctypes.data_as(C.POINTER(C.c_double))
    if nnz_p:
        keep += [np.ascontiguousarray([i for j in range(n) for i in range(j + 1)], dtype=np.int32), np.ascontiguousarray(np.cumsum([0] + list(range(1, n + 1))), dtype=np.int32)]
        t.nnz_p, t.p_indices, t.p_indptr = int(keep[6][-1]), ip(keep[5]), ip(keep[6])
    return t, keep, tpl


def _plan(host, n, cones, nnz_p=0):
    t, keep, tpl = _template(n, cones, nnz_p)
    out = (C.c_long * 5)()
    assert host.h_plan_tri(C.byref(t), out) == 0
    return dict(zip(("ns_variant", "qp_ns_variant", "tri_ns_variant", "tri_ns_lds", "bwd_mode"), out)), tpl


def _row(host, v):
    a, b = C.c_int(), C.c_int()
    host.h_row(v, C.byref(a), C.byref(b))
    return a.value, b.value


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_tri_footprint_is_the_kernels_carve_and_the_plan_picks_the_expected_row(host, shape, monkeypatch):
    for e in PLAN_ENV:
        monkeypatch.delenv(e, raising=False)
    n, cones, B, seed, row = K.SHAPES[shape]
    plan, tpl = _plan(host, n, cones)
    assert plan["tri_ns_variant"] == row and plan["ns_variant"] == -1 and plan["qp_ns_variant"] == -1 and plan["bwd_mode"] == 3, plan
    ntri, nq = cones.get("ep", 0) + len(cones.get("p", [])), len(cones.get("q", []))
    for v in range(host.h_rows()):
        ntile, nthr = _row(host, v)
        carve = (C.c_long * 3)(); lay = (C.c_long * 12)()
        host.h_carve_tri(n, tpl.m, nq, ntri, ntile, nthr, carve)
        host.h_layout_tri(n, tpl.m, nq, ntri, ntile, nthr, lay)
        assert (lay[0], lay[2]) == (carve[0], carve[1]) and (lay[1], lay[3]) == (72 * ntri, 24 * ntri), (shape, v, list(lay), list(carve))
        assert lay[0] % 8 == 0 and lay[4] == carve[2] and carve[2] <= lay[5] <= carve[2] + 16 and lay[5] == lay[6], (shape, v, list(lay), list(carve))
        assert lay[5] - lay[7] in (96 * ntri, 96 * ntri + 4), (shape, v)          # W and lambda on top of the plain footprint (+ the rounding of the ints to 8 bytes)
        if v == row:
            assert plan["tri_ns_lds"] == lay[5]
        if v < row:          # the rows in front of the chosen one do not hold the reduced system or exceed LDS
            assert 4 * ((n + 3) // 4) + 1 > 16 * ntile or lay[5] > 160 * 1024


def test_plain_and_qp_footprints_are_unchanged(host):
    """the quoted footprints of test_ns_layout_host.py through the new signature; neither mode has a byte of the triples' segments"""
    lay = (C.c_long * 12)()
    host.h_layout_tri(50, 100, 0, 0, 4, 256, lay)
    assert (lay[7], lay[8], lay[10], lay[11]) == (52496, 73096, 52496, 73096) and lay[9] == 0 and lay[5] == lay[7]
    for n, m, nq in ((12, 23, 1), (40, 88, 1), (80, 128, 4), (108, 250, 0)):
        for v in range(host.h_rows()):
            host.h_layout_tri(n, m, nq, 3, *_row(host, v), lay)
            assert lay[9] == 0 and lay[10] == lay[7] and lay[11] == lay[8] and lay[5] > lay[7]


def test_templates_that_get_no_tri_variant(host, monkeypatch):
    for e in PLAN_ENV:
        monkeypatch.delenv(e, raising=False)
    assert _plan(host, 12, {"z": 2, "l": 6, "q": [4, 5]})[0]["tri_ns_variant"] == -1                       # plain cones: ns_variant serves them
    assert _plan(host, 12, {"z": 2, "l": 6, "q": [4, 5]})[0]["ns_variant"] == 0
    assert _plan(host, 6, {"z": 1, "l": 2, "s": [2], "ep": 1})[0]["tri_ns_variant"] == -1                  # a PSD block
    assert _plan(host, 112, {"z": 2, "l": 6, "q": [], "ep": 2})[0]["tri_ns_variant"] == -1                 # n > 108
    assert _plan(host, 108, {"z": 2, "l": 6, "q": [], "ep": 2})[0]["tri_ns_variant"] == 2
    assert _plan(host, 12, {"z": 2, "l": 6, "q": [], "ep": 2}, nnz_p=1)[0]["tri_ns_variant"] == -1         # a quadratic objective
    monkeypatch.setenv("CE_BWD_NS", "0")
    assert _plan(host, 12, {"z": 2, "l": 6, "q": [], "ep": 2})[0]["tri_ns_variant"] == -1


def test_the_query_is_bound_and_argument_handling_is_unchanged():
    L = _lib.lib()
    assert "ce_tri_ns_variant" in _lib.SYMBOLS and L.ce_tri_ns_variant(None) == -1 and L.ce_adjoint_ns_variant(None) == -1
    from cvxpylayers_amd.interfaces.cone_engine import ConeEngine
    from cvxpylayers_amd.interfaces.solver_args import jvp_mode, refine_steps
    assert ConeEngine.PLAN_FIELDS[-1] == "tri_ns_variant" and ConeEngine.PLAN_FIELDS[10] == "ns_variant" and len(ConeEngine.PLAN_FIELDS) == 18
    assert jvp_mode({}) == "lsqr" and jvp_mode({"jvp_mode": "direct"}) == "direct" and jvp_mode({"jvp_mode": "lsqr"}) == "lsqr"
    with pytest.raises(ValueError, match="jvp_mode"):
        jvp_mode({"jvp_mode": "nonsense"})
    assert refine_steps({}) == 0 and refine_steps({"refine_steps": 2}) == 2 and refine_steps({"refine_steps": np.int64(3)}) == 3
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="refine_steps"):
            refine_steps({"refine_steps": bad})
    for doc in (jvp_mode.__doc__, refine_steps.__doc__):
        assert "exponential / power cones" not in doc

"""The served class, the row selection and the LDS footprint of k_newton_wave_qp (cvxpylayers_amd/csrc/ce_lds_newton_wave_qp.h, ce_variants_newton_wave_qp.h) are
plain C++ apart from their qualifiers, so they are checked on the host, compiled with g++: served and refused templates with their reasons, the first-fit row at every
instantiation's bounds and one past them, the footprint (k_bwd_wave_qp's carve to the byte: A, R | B_1^-1, P, two x and two y staging vectors, the equalities' row
indices).  And the five new C entries are bound with the workgroup entries' argument types, answer -1 / 0 / 0 on a NULL handle, and the object is in the Makefile."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cvxpylayers_amd", "csrc")
SRC = r'''
#include <cstddef>
#define __host__
#define __device__
#include "ce_lds_newton_wave_qp.h"
#define X(V, NX, MY, WPS, WPSR) {V, NX, MY, WPS, WPSR},
static const int ROWS[][5] = {CE_NEWTON_WAVE_QP_VARIANTS(X)};
#undef X
extern "C" {
int h_rows() { return (int)(sizeof(ROWS) / sizeof(ROWS[0])); }
void h_row(int v, int *out) { for (int k = 0; k < 5; k++) out[k] = ROWS[v][k]; }
int h_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) { return newton_wave_qp_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p); }
long h_lds(int v, int n, int m) { return (long)newton_wave_qp_lds_bytes(v, n, m); }
const char *h_refusal(int n, int m, int ns, int nep, int np, int nnz_p) { return newton_wave_qp_refusal(n, m, ns, nep, np, nnz_p); }
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("newton_wave_qp_host")
    (d / "host.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", str(d / "libhost.so"), str(d / "host.cpp")])
    L = C.CDLL(str(d / "libhost.so"))
    L.h_variant.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] + [C.c_int] * 4
    L.h_lds.restype = C.c_long; L.h_lds.argtypes = [C.c_int] * 3
    L.h_row.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.h_refusal.restype = C.c_char_p; L.h_refusal.argtypes = [C.c_int] * 6
    rows = []
    for v in range(L.h_rows()):
        buf = (C.c_int * 5)()
        L.h_row(v, buf)
        rows.append(tuple(buf))
    L.rows = rows
    return L


def _variant(host, n, m, z=0, q=(), l=None, ns=0, nep=0, np_=0, nnz_p=1):
    q = list(q)
    l = m - z - sum(q) if l is None else l
    return host.h_variant(n, m, z, l, len(q), (C.c_int * max(len(q), 1))(*q), ns, nep, np_, nnz_p)


def test_served_and_refused_templates(host):
    for n, m, kw in ((1, 1, {}), (2, 3, {}), (32, 64, {}), (32, 64, dict(q=[64])), (12, 14, dict(z=2, q=[1, 5]))):
        assert _variant(host, n, m, **kw) >= 0, (n, m, kw)
    assert _variant(host, 4, 6, nnz_p=0) == -1 and b"without a P structure" in host.h_refusal(4, 6, 0, 0, 0, 0)
    assert _variant(host, 33, 64) == -1 and b"n > 32" in host.h_refusal(33, 64, 0, 0, 0, 1)
    assert _variant(host, 32, 65) == -1 and b"m > 64" in host.h_refusal(32, 65, 0, 0, 0, 1)
    assert _variant(host, 4, 6, l=3, ns=1) == -1 and b"PSD" in host.h_refusal(4, 6, 1, 0, 0, 1)
    assert _variant(host, 4, 6, l=3, nep=1) == -1 and b"exponential" in host.h_refusal(4, 6, 0, 1, 0, 1)
    assert _variant(host, 4, 6, l=3, np_=1) == -1 and b"power" in host.h_refusal(4, 6, 0, 0, 1, 1)
    assert _variant(host, 4, 6, l=2) == -1          # cone rows that do not add up to m


def test_first_fit_and_footprint_at_every_shape(host):
    rows = host.rows
    assert [r[:3] for r in rows] == [(0, 8, 16), (1, 16, 32), (2, 32, 64)]
    for v, nx, my, wps, wpsr in rows:
        assert 1 <= wpsr <= wps <= 8          # (the refinement step holds more across the elimination: never more waves than the forward derivative)
        assert _variant(host, nx, my) == v
        assert _variant(host, nx + 1, my) == (-1 if nx == 32 else v + 1) and _variant(host, nx, my + 1) == (-1 if my == 64 else v + 1)
    for n in range(1, 33):
        for m in range(1, 65):
            v = _variant(host, n, m)
            assert v == next(r[0] for r in rows if n <= r[1] and m <= r[2]), (n, m, v)
            nx, my = rows[v][1:3]
            by = host.h_lds(v, n, m)
            assert by == 8 * ((m + nx + n) * (nx + 1) + 2 * nx + 2 * my + (nx + 1) // 2) and by <= 160 * 1024, (n, m, by)          # ce_lds_bwd_wave_qp.h
            assert host.h_lds(v, nx + 1, m) == 0 and host.h_lds(v, n, my + 1) == 0 and host.h_lds(-1, n, m) == 0 and host.h_lds(len(rows), n, m) == 0
    assert host.h_lds(len(rows) - 1, 32, 64) == 35456


def test_entries_are_bound_answer_a_null_handle_and_the_object_is_built():
    from cvxpylayers_amd import _lib
    L = _lib.lib()
    assert L.ce_jvp_qp_wave.argtypes == L.ce_jvp_qp.argtypes and L.ce_refine_qp_wave.argtypes == L.ce_refine_qp.argtypes
    assert L.ce_newton_wave_qp_variant(None) == -1 and L.ce_newton_wave_qp_lds(None) == 0
    assert L.ce_newton_wave_qp_occupancy(None, 0) == 0 and L.ce_newton_wave_qp_occupancy(None, 1) == 0
    assert L.ce_jvp_qp_wave(None, 1, None, 0, *([None] * 5), 0, None, 0, 0, *([None] * 7)) == -1 and b"ce_jvp_qp_wave" in L.ce_last_error()
    assert L.ce_refine_qp_wave(None, 1, None, 0, None, 0, 0, *([None] * 5), 1, *([None] * 4)) == -1 and b"ce_refine_qp_wave" in L.ce_last_error()
    objs = re.search(r"^OBJS\s*=((?:.*\\\n)*.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    assert "$(OBJDIR)/newton_wave_qp.o" in objs.split()

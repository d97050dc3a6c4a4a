"""The served class, the row selection and the LDS footprint of k_bwd_wave_qp (cvxpylayers_amd/csrc/ce_lds_bwd_wave_qp.h, ce_variants_bwd_wave_qp.h) are plain C++
apart from their qualifiers, so they are checked on the host, compiled with g++: served and refused templates, the first-fit row at every instantiation's bounds and
one past them, the footprint (k_bwd_wave's -- A, R | B_1^-1, two x and two y staging vectors, the equalities' row indices -- plus the n rows of P) within the 160 KB
the other footprints use.  And the new C entries are bound and answer -1 / 0 on a NULL handle."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cvxpylayers_amd", "csrc")
SRC = r'''
#include <cstddef>
#define __host__
#define __device__
#include "ce_lds_bwd_wave_qp.h"
#define X(V, NX, MY, WPS) {V, NX, MY, WPS},
static const int ROWS[][4] = {CE_BWD_WAVE_QP_VARIANTS(X)};
#undef X
extern "C" {
int h_rows() { return (int)(sizeof(ROWS) / sizeof(ROWS[0])); }
void h_row(int v, int *out) { for (int k = 0; k < 4; k++) out[k] = ROWS[v][k]; }
int h_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) { return bwd_wave_qp_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p); }
long h_lds(int v, int n, int m) { return (long)bwd_wave_qp_lds_bytes(v, n, m); }
const char *h_refusal(int n, int m, int ns, int nep, int np, int nnz_p) { return bwd_wave_qp_refusal(n, m, ns, nep, np, nnz_p); }
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bwd_wave_qp_host")
    (d / "host.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", str(d / "libhost.so"), str(d / "host.cpp")])
    L = C.CDLL(str(d / "libhost.so"))
    L.h_variant.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] + [C.c_int] * 4
    L.h_lds.restype = C.c_long; L.h_lds.argtypes = [C.c_int] * 3
    L.h_row.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.h_refusal.restype = C.c_char_p; L.h_refusal.argtypes = [C.c_int] * 6
    rows = []
    for v in range(L.h_rows()):
        buf = (C.c_int * 4)()
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
    for v, nx, my, wps in rows:
        assert 1 <= wps <= 8
        assert _variant(host, nx, my) == v
        assert _variant(host, nx + 1, my) == (-1 if nx == 32 else v + 1) and _variant(host, nx, my + 1) == (-1 if my == 64 else v + 1)
    for n in range(1, 33):
        for m in range(1, 65):
            v = _variant(host, n, m)
            assert v == next(r[0] for r in rows if n <= r[1] and m <= r[2]), (n, m, v)
            _, nx, my, _ = rows[v]
            by = host.h_lds(v, n, m)
            bwd_wave = 8 * ((m + nx) * (nx + 1) + 2 * nx + 2 * my + (nx + 1) // 2)          # ce_lds_bwd_wave.h
            assert by == bwd_wave + 8 * n * (nx + 1) and by <= 160 * 1024, (n, m, by)
            assert host.h_lds(v, nx + 1, m) == 0 and host.h_lds(v, n, my + 1) == 0 and host.h_lds(-1, n, m) == 0 and host.h_lds(len(rows), n, m) == 0
    assert host.h_lds(len(rows) - 1, 32, 64) == 35456


def test_entries_are_bound_and_answer_a_null_handle():
    from cvxpylayers_amd import _lib
    L = _lib.lib()
    assert L.ce_vjp_qp_wave.argtypes == L.ce_vjp_qp.argtypes
    assert L.ce_bwd_wave_qp_variant(None) == -1 and L.ce_bwd_wave_qp_lds(None) == 0 and L.ce_bwd_wave_qp_occupancy(None) == 0
    assert L.ce_vjp_qp_wave(None, 1, None, 0, 0, *([None] * 7), 0, 0, None, 0, 0, None, None, None) == -1 and b"null" in L.ce_last_error()

"""The row selection and the LDS footprint of k_newton_wave (cvxpylayers_amd/csrc/ce_lds_newton_wave.h, ce_variants_newton_wave.h), compiled with g++ on the host as
tests/test_bwd_wave_plan_host.py compiles k_bwd_wave's: the served class and the carve are that kernel's, row for row and byte for byte."""
import ctypes as C
import subprocess

import pytest

from test_bwd_wave_plan_host import CSRC, ROWS
from test_bwd_wave_plan_host import host as bwd_host          # noqa: F401  (the fixture of the adjoint's header: the class this one must equal)

SRC = r'''
#include <cstddef>
#define __host__
#define __device__
#include "ce_lds_newton_wave.h"
extern "C" {
int h_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) { return newton_wave_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p); }
long h_lds(int v, int n, int m) { return (long)newton_wave_lds_bytes(v, n, m); }
const char *h_refusal(int n, int m, int ns, int nep, int np, int nnz_p) { return newton_wave_refusal(n, m, ns, nep, np, nnz_p); }
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("newton_wave_host")
    (d / "host.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", str(d / "libhost.so"), str(d / "host.cpp")])
    L = C.CDLL(str(d / "libhost.so"))
    L.h_variant.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] + [C.c_int] * 4
    L.h_lds.restype = C.c_long; L.h_lds.argtypes = [C.c_int] * 3
    L.h_refusal.restype = C.c_char_p; L.h_refusal.argtypes = [C.c_int] * 6
    return L


@pytest.mark.parametrize("n, m, row", [(8, 16, 0), (9, 16, 1), (8, 17, 1), (16, 32, 1), (17, 32, 2), (16, 33, 2), (32, 64, 2), (33, 64, -1), (32, 65, -1), (1, 1, 0)])
def test_row_selection_and_footprint_at_the_row_edges(host, bwd_host, n, m, row):
    q = (C.c_int * 2)(1, max(m - 1, 1))
    args = (n, m, 0, 0, 2, q, 0, 0, 0, 0) if m >= 2 else (n, m, 0, m, 0, (C.c_int * 1)(), 0, 0, 0, 0)
    assert host.h_variant(*args) == row == bwd_host.h_variant(*args)
    if row >= 0:
        nx, my = ROWS[row]
        by = host.h_lds(row, n, m)
        assert by == 8 * (m * (nx + 1) + nx * (nx + 1) + nx + nx + my + my + (nx + 1) // 2) == bwd_host.h_lds(row, n, m)
        assert 0 < by <= 64 * 1024 and host.h_lds(row, nx + 1, m) == 0 and host.h_lds(row, n, my + 1) == 0 and host.h_lds(3, n, m) == 0
    else:
        assert b"wave Newton kernel" in host.h_refusal(n, m, 0, 0, 0, 0)


def test_refusals_name_the_reason(host):
    assert host.h_variant(4, 6, 0, 3, 0, (C.c_int * 1)(), 0, 1, 0, 0) == -1 and b"exponential" in host.h_refusal(4, 6, 0, 1, 0, 0)
    assert b"P structure" in host.h_refusal(4, 6, 0, 0, 0, 4) and b"PSD" in host.h_refusal(4, 6, 1, 0, 0, 0)
    assert max(host.h_lds(2, n, 64) for n in range(1, 33)) == 27008          # the largest carve of the list: six instances per CU by LDS

"""The served class, the row selection and the LDS footprint of k_bwd_wave (cvxpylayers_amd/csrc/ce_lds_bwd_wave.h, ce_variants_bwd_wave.h) are plain C++ apart from
their qualifiers: the kernel carves with them and ce_create selects with them, so they are checked here on the host, compiled with g++."""
import ctypes as C
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cvxpylayers_amd", "csrc")
SRC = r'''
#include <cstddef>
#define __host__
#define __device__
#include "ce_lds_bwd_wave.h"
extern "C" {
int h_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) { return bwd_wave_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p); }
long h_lds(int v, int n, int m) { return (long)bwd_wave_lds_bytes(v, n, m); }
const char *h_refusal(int n, int m, int ns, int nep, int np, int nnz_p) { return bwd_wave_refusal(n, m, ns, nep, np, nnz_p); }
}
'''
ROWS = [(8, 16), (16, 32), (32, 64)]          # (NX, MY) of the variant list


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bwd_wave_host")
    (d / "host.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", str(d / "libhost.so"), str(d / "host.cpp")])
    L = C.CDLL(str(d / "libhost.so"))
    L.h_variant.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] + [C.c_int] * 4
    L.h_lds.restype = C.c_long; L.h_lds.argtypes = [C.c_int] * 3
    L.h_refusal.restype = C.c_char_p; L.h_refusal.argtypes = [C.c_int] * 6
    return L


def _variant(host, n, m, ns=0, nep=0, np_=0, nnz_p=0):
    return host.h_variant(n, m, 0, m - 3 * (nep + np_) - ns, 0, (C.c_int * 1)(), ns, nep, np_, nnz_p)


@pytest.mark.parametrize("n, m, row", [(8, 16, 0), (9, 16, 1), (8, 17, 1), (16, 32, 1), (17, 32, 2), (16, 33, 2), (32, 64, 2), (33, 64, -1), (32, 65, -1), (1, 1, 0)])
def test_row_selection_at_the_bounds(host, n, m, row):
    assert _variant(host, n, m) == row
    q = (C.c_int * 2)(1, m - 1)
    assert m < 2 or host.h_variant(n, m, 0, 0, 2, q, 0, 0, 0, 0) == row          # cones of any dimensions, 1 included


def test_refusals_and_their_reasons(host):
    assert _variant(host, 4, 6, nnz_p=4) == -1 and b"P structure" in host.h_refusal(4, 6, 0, 0, 0, 4)
    assert _variant(host, 4, 6, ns=1) == -1 and b"PSD" in host.h_refusal(4, 6, 1, 0, 0, 0)
    assert _variant(host, 4, 6, nep=1) == -1 and b"exponential" in host.h_refusal(4, 6, 0, 1, 0, 0)
    assert _variant(host, 4, 6, np_=1) == -1 and b"power" in host.h_refusal(4, 6, 0, 0, 1, 0)
    assert b"n > 32" in host.h_refusal(33, 64, 0, 0, 0, 0) and b"m > 64" in host.h_refusal(32, 65, 0, 0, 0, 0)
    assert host.h_variant(4, 6, 0, 2, 0, (C.c_int * 1)(), 0, 0, 0, 0) == -1          # cone rows that do not add up to m


def test_footprint(host):
    for n in range(1, 33):
        for m in range(1, 65):
            v = _variant(host, n, m)
            nx, my = ROWS[v]
            by = host.h_lds(v, n, m)
            # the kernel's carve, in its order: A (m rows of NX + 1), R | B_1^-1 (NX rows), xb, xb2 (NX), yb, yb2 (MY), erow (NX ints, whole doubles)
            assert by == 8 * (m * (nx + 1) + nx * (nx + 1) + nx + nx + my + my + (nx + 1) // 2), (n, m, by)
            assert 0 < by < 64 * 1024 and by % 8 == 0
            assert host.h_lds(v, nx + 1, m) == 0 and host.h_lds(v, n, my + 1) == 0 and host.h_lds(-1, n, m) == 0 and host.h_lds(3, n, m) == 0
    assert host.h_lds(2, 32, 64) == 8 * (96 * 33 + 64 + 128 + 16) == 27008

"""The served class, the row selection, the chunk and the LDS footprint of k_bwd_wave_many_qp (cvxpylayers_amd/csrc/ce_lds_bwd_wave_many_qp.h,
ce_variants_bwd_wave_many_qp.h) are plain C++ apart from their qualifiers: the kernel carves with them and ce_create selects with them, so they are checked here on
the host, compiled with g++ (as tests/test_bwd_wave_many_plan_host.py checks k_bwd_wave_many's)."""
import ctypes as C
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cvxpylayers_amd", "csrc")
SRC = r'''
#include <cstddef>
#define __host__
#define __device__
#include "ce_lds_bwd_wave_many_qp.h"
extern "C" {
int h_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) { return bwd_wave_many_qp_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p); }
int h_single(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) { return bwd_wave_qp_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p); }
long h_lds(int v, int n, int m) { return (long)bwd_wave_many_qp_lds_bytes(v, n, m); }
int h_chunk(int v) { return bwd_wave_many_qp_chunk(v); }
const char *h_refusal(int n, int m, int ns, int nep, int np, int nnz_p) { return bwd_wave_many_qp_refusal(n, m, ns, nep, np, nnz_p); }
}
'''
ROWS = [(8, 16), (16, 32), (32, 64)]          # (NX, MY): k_bwd_wave_qp's


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bwd_wave_many_qp_host")
    (d / "host.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", str(d / "libhost.so"), str(d / "host.cpp")])
    L = C.CDLL(str(d / "libhost.so"))
    L.h_variant.argtypes = L.h_single.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] + [C.c_int] * 4
    L.h_lds.restype = C.c_long; L.h_lds.argtypes = [C.c_int] * 3
    L.h_refusal.restype = C.c_char_p; L.h_refusal.argtypes = [C.c_int] * 6
    return L


def test_served_class_is_the_single_cotangent_kernels(host):
    q0, q2 = (C.c_int * 1)(), (C.c_int * 2)()
    for n in (1, 8, 9, 16, 17, 32, 33):
        for m in (1, 2, 16, 17, 32, 33, 64, 65):
            for ns, nep, np_, nnz_p in ((0, 0, 0, 4), (1, 0, 0, 4), (0, 1, 0, 4), (0, 0, 1, 4), (0, 0, 0, 0)):
                args = (n, m, 0, m - 3 * (nep + np_) - ns, 0, q0, ns, nep, np_, nnz_p)
                assert host.h_variant(*args) == host.h_single(*args), args
            if m >= 2:
                q2[0], q2[1] = 1, m - 1
                assert host.h_variant(n, m, 0, 0, 2, q2, 0, 0, 0, 4) == host.h_single(n, m, 0, 0, 2, q2, 0, 0, 0, 4)
    assert host.h_variant(4, 6, 0, 6, 0, q0, 0, 0, 0, 4) == 0 and host.h_variant(4, 6, 0, 2, 0, q0, 0, 0, 0, 4) == -1          # cone rows that do not add up to m
    assert b"without a P structure" in host.h_refusal(4, 6, 0, 0, 0, 0) and b"n > 32" in host.h_refusal(33, 64, 0, 0, 0, 4)


def test_chunk_and_footprint(host):
    q0 = (C.c_int * 1)()
    assert [host.h_chunk(v) for v in (-1, 0, 1, 2, 3)] == [0, 8, 16, 8, 0]
    for v, (nx, my) in enumerate(ROWS):
        assert 1 <= host.h_chunk(v) <= 64 - nx          # the right-hand sides ride in the lanes behind the columns
    for n in range(1, 33):
        for m in range(1, 65):
            v = host.h_variant(n, m, 0, m, 0, q0, 0, 0, 0, 4)
            nx, my = ROWS[v]
            kp = host.h_chunk(v) | 1
            by = host.h_lds(v, n, m)
            # the kernel's carve, in its order: A (m rows of NX + 1), R | B_1^-1 (NX rows), P (n rows), xb, xb2 (NX), yb, yb2 (MY), erow (NX ints, whole doubles),
            # then the panels D, T (m rows of KC | 1 each) and FX, DT (NX rows each)
            assert by == 8 * (m * (nx + 1) + nx * (nx + 1) + n * (nx + 1) + nx + nx + my + my + (nx + 1) // 2 + m * kp + m * kp + nx * kp + nx * kp), (n, m, by)
            assert 0 < by < 64 * 1024 and by % 8 == 0          # a launch without a function attribute
            assert host.h_lds(v, nx + 1, m) == 0 and host.h_lds(v, n, my + 1) == 0 and host.h_lds(-1, n, m) == 0 and host.h_lds(3, n, m) == 0
    assert host.h_lds(2, 32, 64) == 35456 + 8 * 192 * 9 == 49280


def test_entries_are_bound_answer_a_null_handle_and_have_their_object():
    from cvxpylayers_amd import _lib
    L = _lib.lib()
    assert L.ce_vjp_qp_many_wave.argtypes == L.ce_vjp_qp_many.argtypes and L.ce_vjp_qp_many_params_wave.argtypes == L.ce_vjp_qp_many_params.argtypes
    assert (L.ce_bwd_wave_many_qp_variant(None), L.ce_bwd_wave_many_qp_lds(None), L.ce_bwd_wave_many_qp_chunk(None), L.ce_bwd_wave_many_qp_occupancy(None)) == (-1, 0, 0, 0)
    assert L.ce_vjp_qp_many_wave(None, 1, 1, None, 0, *([None] * 11)) == -1 and b"ce_vjp_qp_many_wave: null" in L.ce_last_error()
    assert L.ce_vjp_qp_many_params_wave(None, 1, 1, None, 0, *([None] * 6), 0, *([None] * 8)) == -1 and b"ce_vjp_qp_many_params_wave: null" in L.ce_last_error()
    objs = re.search(r"^OBJS\s*=((?:.*\\\n)*.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    assert "$(OBJDIR)/bwd_wave_many_qp.o" in objs.split()

"""k_jvp_wave_many on the host: the row selection, the chunk and the LDS footprint (cvxpylayers_amd/csrc/ce_lds_jvp_wave_many.h, ce_variants_jvp_wave_many.h: plain
C++ apart from their qualifiers, compiled with g++ as tests/test_bwd_wave_many_plan_host.py compiles the sibling's) against the kernel's carve written out; the new
symbols declared and bound under ABI 17; what ce_jvp_many_wave and ConeEngine.jvp_many(wave=True) refuse before they touch a device."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from cvxpylayers_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cvxpylayers_amd", "csrc")
SRC = r'''
#include <cstddef>
#define __host__
#define __device__
#include "ce_lds_jvp_wave_many.h"
extern "C" {
int h_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) { return jvp_wave_many_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p); }
int h_single(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) { return newton_wave_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p); }
long h_lds(int v, int n, int m) { return (long)jvp_wave_many_lds_bytes(v, n, m); }
int h_chunk(int v) { return jvp_wave_many_chunk(v); }
}
'''
ROWS = [(8, 16), (16, 32), (32, 64)]          # (NX, MY): k_newton_wave's
NEW = ["ce_jvp_many_wave", "ce_jvp_wave_many_variant", "ce_jvp_wave_many_lds", "ce_jvp_wave_many_chunk", "ce_jvp_wave_many_occupancy"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("jvp_wave_many_host")
    (d / "host.cpp").write_text(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, "-o", str(d / "libhost.so"), str(d / "host.cpp")])
    L = C.CDLL(str(d / "libhost.so"))
    L.h_variant.argtypes = L.h_single.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] + [C.c_int] * 4
    L.h_lds.restype = C.c_long; L.h_lds.argtypes = [C.c_int] * 3
    return L


@pytest.mark.parametrize("v", [0, 1, 2])
def test_footprint_is_the_kernels_carve(host, v):
    q0 = (C.c_int * 1)()
    nx, my = ROWS[v]
    kc = host.h_chunk(v)
    assert kc == [8, 16, 16][v] and 1 <= kc <= 64 - nx          # the right-hand sides ride in the lanes behind the columns
    kp = kc | 1
    for n, m in ((1, 1), (nx, my)):
        # the kernel's carve, in its order: A (m rows of NX + 1), R | B_1^-1 (NX rows), xb, xb2 (NX), yb, yb2 (MY), erow (NX ints, whole doubles), then the panels
        # GY, T (m rows of KC | 1 each) and FX, DT (NX rows each)
        assert host.h_lds(v, n, m) == 8 * (m * (nx + 1) + nx * (nx + 1) + nx + nx + my + my + (nx + 1) // 2 + m * kp + m * kp + nx * kp + nx * kp), (n, m)
        assert host.h_lds(v, n, m) <= 64 * 1024          # no function attribute on the launch
    assert host.h_lds(v, nx + 1, my) == 0 and host.h_lds(v, nx, my + 1) == 0 and host.h_lds(v, 0, 1) == 0 and host.h_lds(3, 1, 1) == 0 and host.h_chunk(3) == 0
    for n, m in ((nx, my), (nx + 1, my), (nx, my + 1)):          # the row's bounds and one past them: k_newton_wave's selection
        assert host.h_variant(n, m, 0, m, 0, q0, 0, 0, 0, 0) == host.h_single(n, m, 0, m, 0, q0, 0, 0, 0, 0) == (v if (n, m) == (nx, my) else (v + 1 if v < 2 else -1))
    assert host.h_variant(4, 7, 0, 4, 0, q0, 0, 1, 0, 0) == -1          # an exponential cone


def test_symbols_are_declared_and_bound_and_bad_arguments_are_refused_without_a_device():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert set(NEW) <= set(_lib.SYMBOLS) and all(f"int {s}(" in header for s in NEW)
    assert L.ce_abi_version() == _lib.ABI_VERSION == 17 and "#define CE_ABI_VERSION 17" in header
    assert [getattr(L, s)(None) for s in NEW[1:]] == [-1, 0, 0, 0]
    buf = (C.c_double * 4)(); ibuf = (C.c_int * 4)()
    p, ip = C.addressof(buf), C.addressof(ibuf)
    tail = (p, p, p, ip, ip, 1e-8, 1e-8, 1e8, 0, None)
    for args in ((None, 1, 1, p, 4, None, 0, 0, p, p, p, p, 0, 0, None, 0, 0), (None, 1, 1, p, 4, None, 0, 0, p, p, p, p, 0, -1, None, 0, 0),
                 (None, 1, 0, p, 4, None, 0, 0, p, p, p, p, 0, 0, None, 0, 0)):          # a null handle, a negative batch stride, K = 0
        assert L.ce_jvp_many_wave(*args, *tail) == -1 and b"ce_jvp_many_wave" in L.ce_last_error()          # CE_E_BADARG


def test_engine_refuses_wave_outside_its_conditions_before_the_library_is_called():
    from cvxpylayers_amd.interfaces.cone_engine import ConeEngine
    eng = ConeEngine.__new__(ConeEngine)
    eng._h, eng.device, eng.last_path = None, torch.device("cpu"), "per_instance"
    eng.n, eng.m, eng.nnz_aug, eng.nnz_p = 3, 4, 16, 6
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)      # noqa: E731
    point = (z(2, 16), z(2, 3), z(2, 4), z(2, 4))
    for kw in (dict(method="lsqr"), dict(path="const_a"), dict(P_bm=z(2, 6))):
        with pytest.raises(NotImplementedError, match="ce_jvp_many_wave"):
            eng.jvp_many(*point, None, z(5, 2, 4), wave=True, **{"method": "direct", **kw})

"""The C ABI of the parameter gradient from the factors for the QP / TRI / PSD / PSD + TRI many-cotangent kinds, the composed map's P entries and the dP entry
formula -- without a GPU.

ce_dP_entry (csrc/ce_dA_entry.h) is plain C++ apart from its qualifiers; it is compiled for the host with g++, as test_param_grad_args.py compiles ce_dA_entry, and
held against np.longdouble: -1/2 (r_i x_j + r_j x_i) with one rounded product, one fma and an exact scaling by -1/2 is within 2^-53 |r_j x_i| / 2 (the product's
rounding) + 2^-53 |result| (the fma's) of the exact value."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from cvxpylayers_amd import _lib
from cvxpylayers_amd.interfaces.param_grad import ComposedMaps, compose_maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ce_vjp_qp_many_params", "ce_vjp_tri_many_params", "ce_vjp_psd_many_params", "ce_vjp_psd_tri_many_params"]
SIGN, BIT30 = -2 ** 31, 1 << 30


def test_symbols_header_and_integration_stub_agree():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    L = _lib.lib()
    ver = int(re.search(r"#define CE_ABI_VERSION (\d+)", hdr).group(1))
    assert ver == L.ce_abi_version() == _lib.ABI_VERSION == 17          # additions keep the number
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in NEW:
        assert sym in _lib.SYMBOLS and hasattr(L, sym) and re.search(r"\b" + sym + r"\s*\(", body), sym
        assert sym in hdr.split("#define CE_ABI_VERSION")[0], f"{sym} is not listed in the header's ABI note"
        assert f"L.{sym}(" in doc, sym
    for sym in NEW[1:]:          # the arguments of ce_vjp_many_params
        assert getattr(L, sym).argtypes == L.ce_vjp_many_params.argtypes, sym
        proto = re.search(r"\bint " + sym + r"\s*\((.*?)\);", body, flags=re.S).group(1)
        assert re.sub(r"\s+", " ", proto) == re.sub(r"\s+", " ", re.search(r"\bint ce_vjp_many_params\s*\((.*?)\);", body, flags=re.S).group(1)), sym
    # ce_vjp_qp_many's arguments with the map (rows, ptr, code, k, val) and g in place of dA_vals / dP_vals
    assert len(L.ce_vjp_qp_many_params.argtypes) == len(L.ce_vjp_qp_many.argtypes) + 6 - 2
    assert "ce_param_grad_records" in _lib.SYMBOLS


def test_null_arguments_are_refused_naming_the_entry():
    L = _lib.lib()
    null = lambda fn: [0 if t in (C.c_int, C.c_long) else None for t in fn.argtypes]
    for sym in NEW:
        fn = getattr(L, sym)
        assert fn(*null(fn)) == -1 and sym.encode() in L.ce_last_error(), sym          # CE_E_BADARG before any device call


# structure of [A | b], m = 3, n = 2: column 0 rows (0, 2), column 1 row (1), b rows (0, 1, 2)
IDX, PTR, N, M = np.array([0, 2, 1, 0, 1, 2]), np.array([0, 2, 3, 6]), 2, 3
A_T = sp.csr_array(np.array([[0, 2.0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1.5, 0, 0, 0, -1.0, 0], [0, 0, 3.0, 0, 0, 0]]))
Q_T = sp.csr_array(np.array([[0, 0, 0], [0, 0, 0], [0, 4.0, 0], [0.5, 0, 7.0]]))
pc = lambda i, j: int(np.int32(SIGN) | np.int32(BIT30) | np.int32(i | (j << 15)))


def test_compose_maps_without_a_P_map_is_unchanged():
    want = compose_maps(A_T, Q_T, IDX, PTR, N, M)
    assert want[0].tolist() == [0, 1, 1, 4, 7] and want[2].tolist() == [1, 0, 4, 0, 2, 0, 0] and want[3].tolist() == [2.0, 1.5, -1.0, 4.0, 3.0, 0.5, 7.0]
    for got in (compose_maps(A_T, Q_T, IDX, PTR, N, M, None), compose_maps(A_T, Q_T, IDX, PTR, N, M, P_mapT=None, prow=[0], pcol=[0], p_tri=True, sym_perm=[0])):
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))
    assert (want[1][want[1] < 0] & BIT30 == 0).all()          # a dq code has bit 30 clear
    cm = ComposedMaps(A_T, Q_T, IDX, PTR, N, M)
    assert cm.nnz_p == 0 and cm.rows == 4


def test_compose_maps_appends_P_entries_behind_the_q_entries_one_triangle():
    # upper triangle of a 2 x 2 P in CSC order: (0, 0), (0, 1), (1, 1)
    prow, pcol = [0, 0, 1], [0, 1, 1]
    P_T = sp.csr_array(np.array([[0, 0, 0], [1.0, 0, 0], [0, 3.0, -2.0], [0, 0.25, 0]]))
    ptr, code, kidx, val = compose_maps(A_T, Q_T, IDX, PTR, N, M, P_T, prow, pcol, True)
    assert ptr.tolist() == [0, 1, 2, 7, 11] and ptr.dtype == code.dtype == kidx.dtype == np.int32
    assert code[1] == pc(0, 0) and kidx[1] == 0 and val[1] == 1.0                          # a diagonal entry is not doubled
    assert code[5:7].tolist() == [pc(0, 1), pc(1, 1)] and kidx[5:7].tolist() == [1, 2] and val[5:7].tolist() == [6.0, -2.0]          # (0, 1) stands for both entries: doubled
    assert code[10] == pc(0, 1) and val[10] == 0.5
    assert (code[[1, 5, 6, 10]] < 0).all() and (code[[1, 5, 6, 10]] & BIT30 != 0).all()
    assert [(int(c) & 0x7fff, (int(c) >> 15) & 0x7fff) for c in code[[1, 5, 6]]] == [(0, 0), (0, 1), (1, 1)]
    # the A and q entries stand where they stood
    w = compose_maps(A_T, Q_T, IDX, PTR, N, M)
    keep = np.array([0, 2, 3, 4, 7, 8, 9])
    assert np.array_equal(code[keep], w[1]) and np.array_equal(kidx[keep], w[2]) and np.array_equal(val[keep], w[3])
    # without the one-triangle flag nothing is doubled
    assert compose_maps(A_T, Q_T, IDX, PTR, N, M, P_T, prow, pcol, False)[3][5:7].tolist() == [3.0, -2.0]
    cm = ComposedMaps(A_T, Q_T, IDX, PTR, N, M, P_T, prow, pcol, True)
    assert cm.nnz_p == 3 and cm.rows == 4
    with pytest.raises(ValueError, match="does not belong"):
        compose_maps(A_T, Q_T, IDX, PTR, N, M, P_T, [0, 0], [0, 1], True)
    with pytest.raises(ValueError, match="out of range"):
        compose_maps(A_T, Q_T, IDX, PTR, N, M, P_T, [0, 0, 2], [0, 1, 1], True)
    with pytest.raises(ValueError, match="needs P's structure"):
        compose_maps(A_T, Q_T, IDX, PTR, N, M, P_T)


def test_compose_maps_carries_the_symmetrisation_of_a_full_structure():
    # full 2 x 2 structure in CSC order: (0, 0), (1, 0), (0, 1), (1, 1); entry k pairs with sym_perm[k]
    prow, pcol, perm = [0, 1, 0, 1], [0, 0, 1, 1], [0, 2, 1, 3]
    P_T = sp.csr_array(np.array([[0, 0, 0, 0], [1.0, 0, 0, 0], [0, 3.0, 0, 0], [0, 5.0, 1.0, 0]]))
    ptr, code, kidx, val = compose_maps(A_T, Q_T, IDX, PTR, N, M, P_T, prow, pcol, False, perm)
    assert ptr.tolist() == [0, 1, 2, 7, 12]
    assert code[1] == pc(0, 0) and val[1] == 1.0                                            # the diagonal's two halves fall together
    assert code[5:7].tolist() == [pc(1, 0), pc(0, 1)] and kidx[5:7].tolist() == [1, 2] and val[5:7].tolist() == [1.5, 1.5]          # the symmetrisation's two entries
    assert code[10:12].tolist() == [pc(1, 0), pc(0, 1)] and val[10:12].tolist() == [3.0, 3.0]          # entries on both sides of a pair: (5 + 1) / 2 each
    # the composed values are the transposed symmetrisation: M' = (M + M[:, perm]) / 2
    Md = P_T.toarray()
    want = 0.5 * (Md + Md[:, perm])
    got = np.zeros_like(Md)
    for r in range(4):
        for t in range(ptr[r], ptr[r + 1]):
            if code[t] < 0 and code[t] & BIT30:
                got[r, kidx[t]] += val[t]
    assert np.array_equal(got, want)


HOST_SRC = r"""
#include <cmath>
#define __device__
#define __forceinline__ inline
#include "ce_dA_entry.h"
extern "C" void entries(int cnt, const double *ri, const double *xj, const double *rj, const double *xi, double *dP) {
    for (int i = 0; i < cnt; i++) dP[i] = ce_dP_entry(ri[i], xj[i], rj[i], xi[i]);
}
"""


def test_dP_entry_on_the_host_against_longdouble(tmp_path):
    (tmp_path / "e.cpp").write_text(HOST_SRC)
    so = str(tmp_path / "e.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "cvxpylayers_amd", "csrc"), "-o", so, str(tmp_path / "e.cpp")])
    lib = C.CDLL(so)
    rng = np.random.default_rng(0)
    Nn = 4000
    ri, xj, rj, xi = (rng.standard_normal(Nn) * 10.0 ** rng.integers(-3, 4, Nn) for _ in range(4))
    # special values: the diagonal (i == j: both products are the same), the zero cotangent (r = 0), x = 0, exact cancellation
    ri[:500] = rj[:500]; xj[:500] = xi[:500]
    ri[500:600] = 0.0; rj[500:600] = 0.0
    xi[600:700] = 0.0
    ri[700:800] = 3.0; xj[700:800] = 2.0; rj[700:800] = -1.5; xi[700:800] = 4.0
    dP = np.empty(Nn)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    lib.entries(Nn, p(ri), p(xj), p(rj), p(xi), p(dP))
    Ld = np.longdouble
    u = Ld(2.0) ** -53
    ril, xjl, rjl, xil = (a.astype(Ld) for a in (ri, xj, rj, xi))
    want = -(ril * xjl + rjl * xil) / 2
    assert (np.abs(dP.astype(Ld) - want) <= u * np.abs(rjl * xil) / 2 + u * np.abs(want) + Ld(5e-324)).all()
    assert (dP[500:600] == 0.0).all() and (dP[700:800] == 0.0).all()
    assert (dP[600:700] == -0.5 * (ri[600:700] * xj[600:700])).all()          # x_i = 0: one rounded product, scaled exactly
    assert (np.abs(dP[:500].astype(Ld) + ril[:500] * xjl[:500]) <= 2 * u * np.abs(ril[:500] * xjl[:500])).all()          # the diagonal: -r_i x_i
    kern = open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "ce_param_grad.h")).read()
    adj = open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "ce_backward_ns.h")).read()
    assert "ce_dP_entry(" in kern and "ce_dP_entry(" in adj          # one statement of the formula, called from both kernels

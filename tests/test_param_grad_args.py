"""solver_args param_grad, the C ABI of the parameter gradient from the adjoint's factors, the composed map and the kernel's entry formulas -- without a GPU.

The entry formulas (csrc/ce_dA_entry.h: ce_dA_entry, ce_db_entry) are plain C++ apart from their qualifiers; they are compiled for the host with g++, as
tests/test_expcone_host.py compiles its headers, and held against np.longdouble: -(x v - y r) with one rounded product and one fma is within 2^-53 |y r| + 2^-53
|result| of the exact value (the product's rounding, then the fma's), y r_tau - v with one fma within 2^-53 |result|."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from cvxpylayers_amd import _lib
from cvxpylayers_amd.interfaces.param_grad import ComposedMaps, compose_maps
from cvxpylayers_amd.interfaces.solver_args import _KNOWN_ARGS, make_settings, param_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ce_vjp_many_params", "ce_vjp_params", "ce_param_grad_variant", "ce_param_grad_records"]


def test_the_key_is_validated():
    assert "param_grad" in _KNOWN_ARGS
    assert param_grad({}) == "dA" and param_grad({"param_grad": "dA"}) == "dA" and param_grad({"param_grad": "factors"}) == "factors"
    for bad in ("Factors", "da", "", None, 1, True, ["factors"]):
        with pytest.raises(ValueError, match="param_grad must be 'dA' or 'factors'"):
            param_grad({"param_grad": bad})
    make_settings({"param_grad": "factors", "eps": 1e-6})          # (a known key: the settings do not read it)


def test_a_wrong_value_raises_before_the_device_is_touched(monkeypatch):
    """forward and jacobian validate the key first: on a host without a GPU the ValueError comes, not the "no CPU fallback" RuntimeError"""
    import torch
    from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    tpl = template_from_affine_builder(lambda b: (np.array([[-1.0], [1.0]]), np.array([b[0], 1.0]), np.array([1.0])), [(1,)], {"z": 0, "l": 2, "q": []},
                                       [VariableRecovery(slice(0, 1), None, (1,))])
    layer = CvxpyLayer(template=tpl)
    p = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    for call in (layer, layer.jacobian):
        with pytest.raises(ValueError, match="param_grad must be"):
            call(p, solver_args={"param_grad": "factor"})
    with pytest.raises(ValueError, match="param_grad must be"):
        CvxpyLayer(template=tpl, solver_args={"param_grad": "rows"})(p)


def test_symbols_and_abi_version():
    """additions that leave every existing call as it was keep CE_ABI_VERSION (the header's rule): header, library, binding and the INTEGRATION.md stub agree"""
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    L = _lib.lib()
    ver = int(re.search(r"#define CE_ABI_VERSION (\d+)", hdr).group(1))
    assert ver == L.ce_abi_version() == _lib.ABI_VERSION
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"ce_abi_version() == {ver}" in doc
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in NEW:
        assert sym in _lib.SYMBOLS and hasattr(L, sym) and re.search(r"\b" + sym + r"\s*\(", body), sym
        assert sym in hdr.split("#define CE_ABI_VERSION")[0], f"{sym} is not listed in the header's ABI note"
    for sym in NEW[:2]:
        assert f"L.{sym}(" in doc, sym
    assert len(L.ce_vjp_many_params.argtypes) == len(L.ce_vjp_many.argtypes) + 5 and len(L.ce_vjp_params.argtypes) == len(L.ce_vjp.argtypes) + 5 - 2
    assert L.ce_param_grad_variant(None) == -1
    null = lambda fn: [0 if t in (C.c_int, C.c_long) else None for t in fn.argtypes]
    assert L.ce_vjp_many_params(*null(L.ce_vjp_many_params)) == -1 and b"ce_vjp_many_params" in L.ce_last_error()          # CE_E_BADARG before any device call
    assert L.ce_vjp_params(*null(L.ce_vjp_params)) == -1 and b"ce_vjp_params" in L.ce_last_error()


def test_the_kernel_has_an_object_of_its_own_and_no_variant_row():
    mk = open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "Makefile")).read()
    assert "$(OBJDIR)/param_grad.o: ce_tu_param_grad.hip" in mk and mk.count("$(OBJDIR)/param_grad.o") == 2
    assert "param_grad" not in open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "ce_variants.h")).read()
    kern = open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "ce_param_grad.h")).read()
    assert "ce_dA_entry(" in kern and "ce_db_entry(" in kern and '#include "ce_dA_entry.h"' in kern


def test_compose_maps_packs_both_maps_per_parameter_row():
    # structure of [A | b], m = 3, n = 2: column 0 rows (0, 2), column 1 row (1), b rows (0, 1, 2)
    indices, indptr, n, m = np.array([0, 2, 1, 0, 1, 2]), np.array([0, 2, 3, 6]), 2, 3
    A_T = sp.csr_array(np.array([[0, 2.0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1.5, 0, 0, 0, -1.0, 0], [0, 0, 3.0, 0, 0, 0]]))
    q_T = sp.csr_array(np.array([[0, 0, 0], [0, 0, 0], [0, 4.0, 0], [0.5, 0, 7.0]]))
    ptr, code, kidx, val = compose_maps(A_T, q_T, indices, indptr, n, m)
    assert ptr.tolist() == [0, 1, 1, 4, 7] and ptr.dtype == code.dtype == kidx.dtype == np.int32 and val.dtype == np.float64
    ij = lambda i, j: i | (j << 16)
    qf = lambda j: int(np.int32(j) | np.int32(-2 ** 31))
    assert code.tolist() == [ij(2, 0), ij(0, 0), ij(1, 2), qf(1), ij(1, 1), qf(0), qf(2)]
    assert kidx.tolist() == [1, 0, 4, 0, 2, 0, 0] and val.tolist() == [2.0, 1.5, -1.0, 4.0, 3.0, 0.5, 7.0]
    assert (code[[3, 5, 6]] < 0).all() and (code[[3, 5, 6]] & 0x7fffffff).tolist() == [1, 0, 2]
    cm = ComposedMaps(A_T, q_T, indices, indptr, n, m)
    assert (cm.rows, cm.n, cm.m, cm.nnz_aug) == (4, 2, 3, 6)
    with pytest.raises(ValueError, match="do not belong"):
        compose_maps(A_T, q_T, indices, indptr, 3, m)
    with pytest.raises(ValueError, match="m < 65536"):
        compose_maps(A_T, q_T, indices, indptr, n, 1 << 16)


HOST_SRC = r"""
#include <cmath>
#define __device__
#define __forceinline__ inline
#include "ce_dA_entry.h"
extern "C" void entries(int cnt, const double *x, const double *v, const double *y, const double *r, const double *rt, double *dA, double *db) {
    for (int i = 0; i < cnt; i++) { dA[i] = ce_dA_entry(x[i], v[i], y[i], r[i]); db[i] = ce_db_entry(y[i], rt[i], v[i]); }
}
"""


def test_entry_formulas_on_the_host_against_longdouble(tmp_path):
    (tmp_path / "e.cpp").write_text(HOST_SRC)
    so = str(tmp_path / "e.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "cvxpylayers_amd", "csrc"), "-o", so, str(tmp_path / "e.cpp")])
    lib = C.CDLL(so)
    rng = np.random.default_rng(0)
    N = 4000
    x, v, y, r, rt = (rng.standard_normal(N) * 10.0 ** rng.integers(-3, 4, N) for _ in range(5))
    # special values: r_tau = 0 (the elimination), x = 0, y = 0, cancellation x v == y r, zero cotangent
    rt[:500] = 0.0; x[500:600] = 0.0; y[600:700] = 0.0
    x[700:800] = 3.0; v[700:800] = 2.0; y[700:800] = 1.5; r[700:800] = 4.0
    v[800:900] = 0.0; r[800:900] = 0.0
    dA, db = np.empty(N), np.empty(N)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    lib.entries(N, p(x), p(v), p(y), p(r), p(rt), p(dA), p(db))
    Ld = np.longdouble
    u = Ld(2.0) ** -53
    xl, vl, yl, rl, tl = (a.astype(Ld) for a in (x, v, y, r, rt))
    want_A, want_b = -(xl * vl - yl * rl), yl * tl - vl
    assert (np.abs(dA.astype(Ld) - want_A) <= u * np.abs(yl * rl) + u * np.abs(want_A) + Ld(5e-324)).all()
    assert (np.abs(db.astype(Ld) - want_b) <= u * np.abs(want_b) + Ld(5e-324)).all()
    assert (db[:500] == -v[:500]).all()                       # r_tau = 0: the -v the elimination's row holds
    assert (dA[500:600] == y[500:600] * r[500:600]).all()     # x = 0: the one rounded product
    assert (dA[700:800] == 0.0).all() and (dA[800:900] == 0.0).all() and (db[800:900] == y[800:900] * rt[800:900]).all()

"""Argument rules of the forward derivative / refinement with a quadratic objective inside the kernels (ce_jvp_qp, ce_refine_qp, ce_qp_ns_variant) that need no
device: what the library refuses before it touches one, and what ConeEngine.jvp and _ConeLayer.jvp refuse before they call it.  The kernels themselves are
tests/test_gpu_qp_jvp.py and tests/test_gpu_qp_refine.py."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from cvxpylayers_amd import _lib


def test_the_new_entry_points_are_bound_and_refuse_null_arguments_without_a_device():
    L = _lib.lib()
    assert {"ce_jvp_qp", "ce_refine_qp", "ce_qp_ns_variant"} <= set(_lib.SYMBOLS)
    assert L.ce_abi_version() == _lib.ABI_VERSION == 17
    assert L.ce_qp_ns_variant(None) == -1 and L.ce_qp_native(None) == 0
    buf = (C.c_double * 4)(); ibuf = (C.c_int * 4)()
    p, ip = C.addressof(buf), C.addressof(ibuf)
    assert L.ce_jvp_qp(None, 1, p, 0, p, p, p, p, None, 0, None, 0, 0, None, p, p, None, ip, None, None) == -1          # CE_E_BADARG
    assert b"null argument" in L.ce_last_error()
    assert L.ce_refine_qp(None, 1, p, 0, p, 1, 1, p, p, p, p, None, 1, ip, ip, p, None) == -1
    assert b"ce_refine_qp" in L.ce_last_error()


def _bare_engine():
    """a ConeEngine without a handle: enough for the argument checks that run before the library is called"""
    from cvxpylayers_amd.interfaces.cone_engine import ConeEngine
    eng = ConeEngine.__new__(ConeEngine)
    eng._h = None
    eng.device = torch.device("cpu")
    eng.last_path = "per_instance"
    eng.n, eng.m, eng.nnz_aug, eng.nnz_p = 3, 4, 16, 6
    return eng


def test_engine_jvp_with_P_needs_the_direct_method():
    eng = _bare_engine()
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)      # noqa: E731
    with pytest.raises(NotImplementedError, match="method='direct'"):
        eng.jvp(z(2, 16), z(2, 3), z(2, 4), z(2, 4), None, None, P_bm=z(2, 6))
    with pytest.raises(ValueError, match="method"):
        eng.jvp(z(2, 16), z(2, 3), z(2, 4), z(2, 4), None, None, P_bm=z(2, 6), method="nonsense")
    # an empty batch launches nothing, with or without P
    out = eng.jvp(z(0, 16), z(0, 3), z(0, 4), z(0, 4), None, None, P_bm=z(0, 6), method="direct")
    assert [tuple(t.shape) for t in out] == [(0, 3), (0, 4), (0, 4), (0,)]
    x, y, s, info = eng.refine(z(0, 16), z(4, 0), z(0, 3), z(0, 4), z(0, 4), 2, P_bm=z(0, 6))
    assert info["path"] == "none" and x.shape == (0, 3)


def test_layer_jvp_with_native_P_refuses_the_default_mode_and_names_both_ways_out():
    from cvxpylayers_amd.interfaces.mi355_if import _ConeLayer, _Saved
    P_bm = torch.zeros((2, 6), dtype=torch.float64)
    saved = _Saved(_bare_engine(), None, None, None, None, False, P_bm, "per_instance", None, (1e-8, 1e-8, 0), None, "lsqr")
    ctx = SimpleNamespace(backward_data=(saved, 2, False, torch.device("cpu")), info={})
    with pytest.raises(NotImplementedError) as e:
        _ConeLayer.jvp(ctx, torch.zeros((6, 2), dtype=torch.float64), None, None)
    assert "CE_QP_EPIGRAPH" in str(e.value) and "jvp_mode='direct'" in str(e.value)
    # no tangent at all: nothing to do, in either mode
    direct = saved._replace(jvp_mode="direct")
    ctx = SimpleNamespace(backward_data=(direct, 2, False, torch.device("cpu")), info={})
    assert _ConeLayer.jvp(ctx, None, None, None) == (None, None, None, None)

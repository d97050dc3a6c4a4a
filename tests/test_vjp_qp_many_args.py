"""Host side of the many-cotangent adjoint with a quadratic objective inside the kernels (no device): ce_vjp_qp_many and ce_vjp_qp_many_variant are declared, bound
and exported under the unchanged ABI version, refuse bad arguments before any device call, and solver_args qp_adjoint takes its two values and no third.

The mode adds no layout mode: it rebuilds every cotangent's vectors in the buffers of ce_jvp_qp (ce_ns_layout.h is untouched; the plan table and
tests/test_ns_layout_host.py pin it).  Non-contiguous A rows need a template's row length, that is an engine, that is a device: tests/test_gpu_vjp_qp_many.py."""
import ctypes as C
import os
import re

import pytest

from cvxpylayers_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ce_vjp_qp_many", "ce_vjp_qp_many_variant")


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert re.search(r"\bint ce_vjp_qp_many\(ce_handle h, int B, int K,", hdr) and re.search(r"\bint ce_vjp_qp_many_variant\(ce_handle h\);", hdr)
    assert "ce_vjp_qp_many and ce_vjp_qp_many_variant" in hdr          # (named in the ABI history under 17)
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    assert len(L.ce_vjp_qp_many.argtypes) == 16 and len(L.ce_vjp_qp_many_variant.argtypes) == 1
    assert L.ce_vjp_qp_many_variant(None) == -1


def test_abi_version_stays_17():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert int(re.search(r"#define CE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == _lib.lib().ce_abi_version() == _lib.ABI_VERSION


def _call(L, h, B, K, p, **null):
    a = dict(A=p, P=p, x=p, y=p, s=p, dx=p, dy=p, dA=p, dq=p, dP=p, st=p)
    a.update(null)
    return L.ce_vjp_qp_many(h, B, K, a["A"], 1, a["P"], a["x"], a["y"], a["s"], a["dx"], a["dy"], a["dA"], a["dq"], a["dP"], a["st"], None)


def test_bad_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert _call(L, None, 1, 1, p) == -1 and b"ce_vjp_qp_many" in L.ce_last_error()          # CE_E_BADARG: null handle
    # K <= 0, B <= 0, a null required pointer: refused on the arguments alone (the handle is never looked at: a block of zeros stands for it)
    fake = (C.c_char * 4096)()
    h = C.addressof(fake)
    assert _call(L, h, 1, 0, p) == -1 and _call(L, h, 1, -3, p) == -1 and _call(L, h, 0, 2, p) == -1 and _call(L, h, -1, 2, p) == -1
    assert b"ce_vjp_qp_many" in L.ce_last_error()
    for name in ("A", "P", "x", "y", "s", "dx", "dA", "dq", "dP"):
        assert _call(L, h, 1, 2, p, **{name: None}) == -1, name


def test_qp_adjoint_takes_its_two_values_and_no_third():
    from cvxpylayers_amd.interfaces import solver_args as SA
    assert "qp_adjoint" in SA._KNOWN_ARGS
    assert SA.qp_adjoint({}) == "pivoting" and SA.qp_adjoint({"qp_adjoint": "pivoting"}) == "pivoting" and SA.qp_adjoint({"qp_adjoint": "search_free"}) == "search_free"
    for bad in ("searchfree", "", None, 1, "Pivoting"):
        with pytest.raises(ValueError, match="qp_adjoint"):
            SA.qp_adjoint({"qp_adjoint": bad})

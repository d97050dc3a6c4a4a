"""Host side of the many-tangent forward derivative (no device): ce_jvp_many, ce_jvp_qp_many and their *_variant queries are declared, bound and exported under the
unchanged ABI version, refuse bad arguments before any device call, and CvxpyLayer.jacobian refuses a bad direction -- and, under direction="forward", what has no
Jacobian -- before it touches a device.

The modes add no layout mode: they rebuild every tangent's vectors in the buffers of ce_jvp / ce_jvp_qp (ce_ns_layout.h is untouched; the plan table and
tests/test_ns_layout_host.py pin it).  A batch stride between 1 and the row length needs a template's row length, that is an engine, that is a device: refused by
the same test of the argument as the negative stride here, it is exercised with a real engine in tests/test_gpu_jvp_many.py."""
import ctypes as C
import os
import re

import pytest
import torch

from cvxpylayers_amd import _lib
from test_vjp_many_args import _template

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ce_jvp_many", "ce_jvp_qp_many", "ce_jvp_many_variant", "ce_jvp_qp_many_variant")


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert re.search(r"\bint ce_jvp_many\(ce_handle h, int B, int K,", hdr) and re.search(r"\bint ce_jvp_qp_many\(ce_handle h, int B, int K,", hdr)
    assert re.search(r"\bint ce_jvp_many_variant\(ce_handle h\);", hdr) and re.search(r"\bint ce_jvp_qp_many_variant\(ce_handle h\);", hdr)
    assert "ce_jvp_many, ce_jvp_qp_many, ce_jvp_many_variant and ce_jvp_qp_many_variant" in hdr          # (named in the ABI history under 17)
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    assert len(L.ce_jvp_many.argtypes) == 27 and len(L.ce_jvp_qp_many.argtypes) == 24
    assert L.ce_jvp_many_variant(None) == -1 and L.ce_jvp_qp_many_variant(None) == -1


def test_abi_version_stays_17():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert int(re.search(r"#define CE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == _lib.lib().ce_abi_version() == _lib.ABI_VERSION


def _plain(L, h, B, K, p, stA_b=1, stq_b=1, **null):
    a = dict(A=p, x=p, y=p, s=p, dx=p, dy=p, st=p)
    a.update(null)
    return L.ce_jvp_many(h, B, K, a["A"], 1, None, 0, 0, a["x"], a["y"], a["s"], p, 1, stA_b, p, 1, stq_b, a["dx"], a["dy"], None, a["st"], None, 1e-8, 1e-8, 1e8, 0, None)


def _qp(L, h, B, K, p, stA_b=1, stq_b=1, stP_b=1, **null):
    a = dict(A=p, P=p, x=p, y=p, s=p, dx=p, dy=p, st=p)
    a.update(null)
    return L.ce_jvp_qp_many(h, B, K, a["A"], 1, a["P"], a["x"], a["y"], a["s"], p, 1, stA_b, p, 1, stq_b, p, 1, stP_b, a["dx"], a["dy"], None, a["st"], None, None)


def test_bad_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    # K <= 0, B <= 0, a null required pointer, a negative batch stride: refused on the arguments alone (the handle is never looked at: a block of zeros stands for it)
    fake = (C.c_char * 4096)()
    h = C.addressof(fake)
    for call, who, required in ((_plain, b"ce_jvp_many", ("A", "x", "y", "s", "dx", "dy", "st")), (_qp, b"ce_jvp_qp_many", ("A", "P", "x", "y", "s", "dx", "dy", "st"))):
        assert call(L, None, 1, 1, p) == -1 and who in L.ce_last_error()          # CE_E_BADARG: null handle
        assert call(L, h, 1, 0, p) == -1 and call(L, h, 1, -3, p) == -1 and call(L, h, 0, 2, p) == -1 and call(L, h, -1, 2, p) == -1
        for name in required:
            assert call(L, h, 1, 2, p, **{name: None}) == -1, name
        assert call(L, h, 2, 2, p, stA_b=-1) == -1 and b"batch stride" in L.ce_last_error()
        assert call(L, h, 2, 2, p, stq_b=-4) == -1
    assert _qp(L, h, 2, 2, p, stP_b=-1) == -1


def test_jacobian_refuses_a_bad_direction_and_keeps_its_refusals_under_forward():
    from cvxpylayers_amd.torch import CvxpyLayer
    F, g = torch.ones(2, 4, dtype=torch.float64), torch.ones(2, dtype=torch.float64)          # CPU tensors: a device would be asked for only behind the refusals
    layer = CvxpyLayer(template=_template())
    with pytest.raises(ValueError, match="direction"):
        layer.jacobian(F, g, direction="sideways")
    with pytest.raises(ValueError, match="direction"):          # (before the other refusals, too)
        CvxpyLayer(template=_template(gp=True)).jacobian(F, g, direction="sideways")
    for direction in ("forward", "auto"):
        with pytest.raises(NotImplementedError, match="gp=True"):
            CvxpyLayer(template=_template(gp=True)).jacobian(F, g, direction=direction)
        for mode in ("lpgd", "lpgd_left", "lpgd_right"):
            with pytest.raises(NotImplementedError, match="not linear in the cotangent"):
                layer.jacobian(F, g, solver_args={"mode": mode}, direction=direction)
        with pytest.raises(RuntimeError, match="ROCm device"):          # (an ordinary call gets as far as the device check)
            layer.jacobian(F, g, direction=direction)

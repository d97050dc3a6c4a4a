"""Host side of the many-cotangent adjoint (no device): ce_vjp_many / ce_vjp_many_variant are declared, bound and exported under the unchanged ABI version, refuse
bad arguments before any device call, and CvxpyLayer.jacobian refuses what has no Jacobian before it touches a device.

The mode adds no layout mode: it rebuilds every cotangent's vectors in the buffers of the plain adjoint (ce_ns_layout.h is untouched, the plan table and
tests/test_ns_layout_host.py pin it), so there is no footprint of its own to compile and check here; ce_vjp_many_variant reports the plain row."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from cvxpylayers_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert re.search(r"\bint ce_vjp_many\(ce_handle h, int B, int K,", hdr) and re.search(r"\bint ce_vjp_many_variant\(ce_handle h\);", hdr)
    assert "ce_vjp_many and ce_vjp_many_variant" in hdr          # (named in the ABI history under 17)
    assert "ce_vjp_many" in _lib.SYMBOLS and "ce_vjp_many_variant" in _lib.SYMBOLS
    L = _lib.lib()
    assert L.ce_vjp_many is not None and L.ce_vjp_many_variant is not None
    assert len(L.ce_vjp_many.argtypes) == 17 and L.ce_vjp_many_variant(None) == -1


def test_abi_version_stays_17():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert int(re.search(r"#define CE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == _lib.lib().ce_abi_version() == _lib.ABI_VERSION


def test_bad_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert L.ce_vjp_many(None, 1, 1, p, 1, None, 0, 0, p, p, p, p, None, p, p, None, None) == -1          # CE_E_BADARG: null handle
    assert b"ce_vjp_many" in L.ce_last_error()
    # K = 0, B = 0 and a null required pointer: refused on the arguments alone (the handle is never looked at: a block of zeros stands for it)
    fake = (C.c_char * 4096)()
    h = C.addressof(fake)
    assert L.ce_vjp_many(h, 1, 0, p, 1, None, 0, 0, p, p, p, p, None, p, p, None, None) == -1
    assert L.ce_vjp_many(h, 1, -3, p, 1, None, 0, 0, p, p, p, p, None, p, p, None, None) == -1
    assert L.ce_vjp_many(h, 0, 2, p, 1, None, 0, 0, p, p, p, p, None, p, p, None, None) == -1
    assert L.ce_vjp_many(h, 1, 2, p, 1, None, 0, 0, p, p, p, None, None, p, p, None, None) == -1          # dx
    assert L.ce_vjp_many(h, 1, 2, p, 1, None, 0, 0, p, p, p, p, None, None, p, None, None) == -1          # dA_vals


def _template(gp=False):
    import dataclasses
    import kit
    from cvxpylayers_amd.torch import VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder

    def builder(F, g):          # kit.min_norm_eq's rows (its closed form does not exist at the F = 0 the affine probing evaluates)
        k, n = F.shape
        Az = np.zeros((k, n + 1)); Az[:, :n] = F
        A2, b2 = kit._soc_sumsq_rows(np.eye(n), np.zeros(n), n, n + 1)
        c = np.zeros(n + 1); c[n] = 1.0
        return np.vstack([Az, A2]), np.concatenate([g, b2]), c
    tpl = template_from_affine_builder(builder, [(2, 4), (2,)], {"z": 2, "l": 0, "q": [6]}, [VariableRecovery(slice(0, 4), None, (4,))])
    return dataclasses.replace(tpl, gp=True, gp_log_mask=(False, False)) if gp else tpl


def test_jacobian_refuses_gp_layers_and_lpgd_modes_before_touching_a_device():
    from cvxpylayers_amd.torch import CvxpyLayer
    F, g = torch.ones(2, 4, dtype=torch.float64), torch.ones(2, dtype=torch.float64)          # CPU tensors: a device would be asked for only behind the refusals
    with pytest.raises(NotImplementedError, match="gp=True"):
        CvxpyLayer(template=_template(gp=True)).jacobian(F, g)
    layer = CvxpyLayer(template=_template())
    for mode in ("lpgd", "lpgd_left", "lpgd_right"):
        with pytest.raises(NotImplementedError, match="not linear in the cotangent"):
            layer.jacobian(F, g, solver_args={"mode": mode})
    with pytest.raises(NotImplementedError, match="not linear in the cotangent"):
        CvxpyLayer(template=_template(), solver_args={"mode": "lpgd"}).jacobian(F, g)
    with pytest.raises(RuntimeError, match="ROCm device"):          # (an ordinary call gets as far as the device check)
        layer.jacobian(F, g)


def test_vjp_many_cotangent_layout_of_the_test_kit():
    """the cotangent stack of tests/test_gpu_vjp_many.py: draw 0 again at K - 1, zeros at position 1, nothing else touched"""
    from test_gpu_vjp_many import K_BEYOND, ZERO_AT, _draw_of, cotangents
    rng = np.random.default_rng(0)
    bx, by = rng.standard_normal((K_BEYOND, 3, 4)), rng.standard_normal((K_BEYOND, 3, 5))
    for K in (1, 3, K_BEYOND):
        dx, dy = cotangents(K, bx, by)
        assert dx.shape == (K, 3, 4) and dy.shape == (K, 3, 5)
        for k in range(K):
            d = _draw_of(K, k)
            if d is None:
                assert k == ZERO_AT and not dx[k].any() and not dy[k].any()
            else:
                assert (dx[k] == bx[d]).all() and (dy[k] == by[d]).all()
        assert K < 3 or ((dx[K - 1] == dx[0]).all() and (dy[K - 1] == dy[0]).all())

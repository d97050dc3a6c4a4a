"""solver_args forward_kernel (cvxpylayers_amd/interfaces/solver_args.py): its default, its two values, the rejection of others before a device is touched, and that
the key leaves the forward settings alone.  No GPU."""
import ctypes as C

import pytest
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd.interfaces import solver_args as SA


def test_key_is_known_and_defaults_to_the_ordinary_kernels():
    assert "forward_kernel" in SA._KNOWN_ARGS
    assert SA.forward_kernel({}) == "workgroup"
    assert SA.forward_kernel({"forward_kernel": "workgroup"}) == "workgroup" and SA.forward_kernel({"forward_kernel": "wave"}) == "wave"


@pytest.mark.parametrize("bad", ["Wave", "warp", "", None, 1, True, ["wave"]])
def test_other_values_raise_and_name_the_accepted_ones(bad):
    with pytest.raises(ValueError, match="forward_kernel must be 'workgroup' or 'wave'"):
        SA.forward_kernel({"forward_kernel": bad})


def test_key_leaves_the_merged_settings_identical():
    base = {"eps": 1e-7, "max_iters": 1234, "alpha": 1.2, "acceleration_lookback": 1}
    a, b = SA.make_settings(dict(base)), SA.make_settings({**base, "forward_kernel": "wave"})
    assert bytes(a) == bytes(b) and C.sizeof(a) == C.sizeof(_lib.CeSettings)
    assert bytes(SA.make_settings({})) == bytes(SA.make_settings({"forward_kernel": "workgroup"}))


def test_a_wrong_value_raises_from_the_plugin_before_the_device_is_touched():
    """on a host without a GPU the plugin's next statement is its 'no CPU fallback' error: the ValueError comes first"""
    from cvxpylayers_amd import problems as P
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    tpl = P.dense_template(3, {"z": 0, "l": 4, "q": []})
    ctx = MI355_ctx(None, tpl.problem_data_index, tpl.cones)
    with pytest.raises(ValueError, match="forward_kernel"):
        _CvxpyLayer.apply(None, torch.zeros(4, 2, dtype=torch.double), torch.zeros(tpl.nnz_aug, 2, dtype=torch.double), ctx, {"forward_kernel": "fast"}, False, None)


def test_binding_declares_the_entry_points():
    for sym in ("ce_solve_wave", "ce_wave_variant", "ce_wave_lds", "ce_wave_occupancy"):
        assert sym in _lib.SYMBOLS
    L = _lib.lib()
    assert L.ce_solve_wave.argtypes == L.ce_solve.argtypes
    assert L.ce_wave_variant(None) == -1 and L.ce_wave_lds(None) == 0 and L.ce_wave_occupancy(None) == 0

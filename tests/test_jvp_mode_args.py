"""solver_args jvp_mode (interfaces/solver_args.py): which method the forward-mode derivative runs.  No device needed."""
import pytest

from cvxpylayers_amd.interfaces import solver_args as SA


def test_jvp_mode_defaults_to_lsqr_and_accepts_direct():
    assert SA.jvp_mode({}) == "lsqr"
    assert SA.jvp_mode({"eps": 1e-9, "mode": "dense"}) == "lsqr"          # (the adjoint's `mode` does not steer the forward derivative)
    assert SA.jvp_mode({"jvp_mode": "lsqr"}) == "lsqr"
    assert SA.jvp_mode({"jvp_mode": "direct"}) == "direct"


@pytest.mark.parametrize("bad", ["nonsense", "", "Direct", None, 1])
def test_jvp_mode_rejects_anything_else(bad):
    with pytest.raises(ValueError, match="jvp_mode must be 'lsqr' or 'direct'"):
        SA.jvp_mode({"jvp_mode": bad})


def test_jvp_mode_is_a_known_solver_arg():
    s = SA.make_settings({"jvp_mode": "direct", "eps": 1e-7})
    assert s.eps_abs == 1e-7
    with pytest.raises(ValueError, match="unknown solver_args"):
        SA.make_settings({"jvp_modes": "direct"})

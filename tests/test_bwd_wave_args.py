"""solver_args adjoint_kernel: validated on the host before the device is touched (cvxpylayers_amd/interfaces/solver_args.py)."""
import pytest

from cvxpylayers_amd.interfaces import solver_args as SA


def test_adjoint_kernel_values():
    assert SA.adjoint_kernel({}) == "workgroup"
    assert SA.adjoint_kernel({"adjoint_kernel": "workgroup"}) == "workgroup" and SA.adjoint_kernel({"adjoint_kernel": "wave"}) == "wave"
    assert SA.adjoint_kernel({"forward_kernel": "wave"}) == "workgroup"          # independent of the forward's key


@pytest.mark.parametrize("bad", ["Wave", "", None, 1, True, "k_bwd_wave"])
def test_adjoint_kernel_refuses_anything_else(bad):
    with pytest.raises(ValueError, match="adjoint_kernel"):
        SA.adjoint_kernel({"adjoint_kernel": bad})

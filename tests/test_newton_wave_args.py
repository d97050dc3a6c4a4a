"""solver_args newton_kernel: validated like adjoint_kernel, known to the plugin, "workgroup" by default.  Host only."""
import pytest

from cvxpylayers_amd.interfaces import solver_args as SA


def test_newton_kernel_values():
    assert SA.newton_kernel({}) == "workgroup" and SA.newton_kernel({"newton_kernel": "workgroup"}) == "workgroup" and SA.newton_kernel({"newton_kernel": "wave"}) == "wave"
    assert "newton_kernel" in next(v for v in vars(SA).values() if isinstance(v, (set, frozenset)) and "adjoint_kernel" in v)


@pytest.mark.parametrize("bad", ["Wave", "", None, 1, True, "workgroup "])
def test_a_bad_value_raises(bad):
    with pytest.raises(ValueError, match="newton_kernel"):
        SA.newton_kernel({"newton_kernel": bad})

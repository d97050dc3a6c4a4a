"""solver_args refine_steps (Newton refinement behind the forward solve, include/cone_engine.h ce_refine): a known argument, an integer >= 0, default 0."""
import numpy as np
import pytest

from cvxpylayers_amd.interfaces.solver_args import _KNOWN_ARGS, make_settings, refine_steps


def test_refine_steps_is_a_known_solver_argument():
    assert "refine_steps" in _KNOWN_ARGS
    make_settings({"eps": 1e-4, "refine_steps": 3})          # (unknown arguments raise here)
    assert refine_steps({"refine_steps": 3}) == 3 and refine_steps({"refine_steps": np.int64(2)}) == 2 and refine_steps({"refine_steps": 0}) == 0


def test_the_default_is_no_refinement():
    assert refine_steps({}) == 0 and refine_steps({"eps": 1e-4}) == 0


@pytest.mark.parametrize("bad", [-1, 1.5, "x"])
def test_anything_but_an_integer_from_zero_up_is_refused(bad):
    with pytest.raises(ValueError, match="refine_steps"):
        refine_steps({"refine_steps": bad})

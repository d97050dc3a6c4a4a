"""solver_args newton_first (Newton steps in front of the forward solve of a warm-started call, interfaces/newton_first.py): a known argument, an integer >= 0,
default 0; its entry point ce_check_solved is bound, and the additions keep the ABI number.  The numpy statement of the termination test (newton_first_kit.py)
is checked here on points whose three residuals are known in closed form."""
import numpy as np
import pytest

from cvxpylayers_amd import _lib
from cvxpylayers_amd.interfaces.solver_args import _KNOWN_ARGS, make_settings, newton_first
from newton_first_kit import perturb, termination_test


def test_newton_first_is_a_known_solver_argument():
    assert "newton_first" in _KNOWN_ARGS
    make_settings({"eps": 1e-4, "newton_first": 2})          # (unknown arguments raise here)
    assert newton_first({"newton_first": 3}) == 3 and newton_first({"newton_first": np.int64(2)}) == 2 and newton_first({"newton_first": 0}) == 0


def test_the_default_is_off():
    assert newton_first({}) == 0 and newton_first({"eps": 1e-4, "refine_steps": 2}) == 0


@pytest.mark.parametrize("bad", [-1, 1.5, True, "x", None])
def test_anything_but_an_integer_from_zero_up_is_refused(bad):
    with pytest.raises(ValueError, match="newton_first"):
        newton_first({"newton_first": bad})


def test_the_entry_point_is_bound_and_the_abi_number_stays():
    L = _lib.lib()
    assert "ce_check_solved" in _lib.SYMBOLS and L.ce_check_solved.argtypes is not None and len(L.ce_check_solved.argtypes) == 25
    assert L.ce_abi_version() == 17 == _lib.ABI_VERSION
    # a null handle is refused before anything is touched
    assert L.ce_check_solved(None, 1, None, 0, 0, None, 0, 0, None, None, None, 0, None, None, None, None, 1, 1e-6, 1e-6, None, None, None, None, None, None) == -1


def test_the_numpy_statement_on_closed_form_points():
    """min x1 + x2 s.t. x >= 1: x = (1, 1), y = (1, 1), s = 0 is the solution; one shifted entry moves exactly one residual"""
    A = -np.eye(2)[None]; b = -np.ones((1, 2)); c = np.ones((1, 2))
    x = np.ones((1, 2)); y = np.ones((1, 2)); s = np.zeros((1, 2))
    t = termination_test(A, b, c, x, y, s, 1e-6, 1e-6)
    assert t["solved"][0] and (t["resid"] == 0).all()
    t = termination_test(A, b + np.array([[0.0, 1e-3]]), c, x, y, s + np.array([[0.0, 1e-3]]), 1e-6, 1e-6)          # b_r and s_r together: the gap alone
    assert list(t["passed"][0]) == [True, True, False] and abs(t["resid"][0, 2] - 1e-3) < 1e-15
    t = termination_test(A, b, c, x * np.nan, y, s, 1e-6, 1e-6)
    assert not t["solved"][0] and not t["finite"][0]
    assert not termination_test(A, b, c, x, y, s, 1e-6, 1e-6, eligible=[False])["solved"][0]
    Pm = np.eye(2)[None]          # min 1/2 |x|^2 + c^T x: stationarity 1 + 1 - y = 0 at y = 2
    t = termination_test(A, b, c, x, 2 * y, s, 1e-6, 1e-6, Pm=Pm)
    assert t["solved"][0] and (t["resid"] == 0).all()


def test_the_perturbation_recipe_draws_A_b_c_in_that_order():
    A, b, c = np.ones((2, 3, 2)), np.ones((2, 3)), np.ones((2, 2))
    rng = np.random.default_rng(105)
    want = [1 + 1e-3 * rng.standard_normal(t.shape) for t in (A, b, c)]
    for got, w in zip(perturb(A, b, c, 1e-3, 5), want):
        np.testing.assert_array_equal(got, w)

"""solver_args psd_elimination (cvxpylayers_amd/interfaces/solver_args.py): its two values, the rejection of others with a message that names them, and that it
is inert where the template has no PSD block -- no GPU needed."""
import warnings

import pytest

from cvxpylayers_amd.interfaces import solver_args as SA


def test_accepts_its_two_values_and_defaults_to_off():
    assert SA.psd_elimination({}) == "off"
    assert SA.psd_elimination({"psd_elimination": "off"}) == "off"
    assert SA.psd_elimination({"psd_elimination": "search_free"}) == "search_free"
    assert "psd_elimination" in SA._KNOWN_ARGS


@pytest.mark.parametrize("bad", ["on", "direct", True, 1, None, "Search_Free"])
def test_rejects_other_values_and_names_them(bad):
    with pytest.raises(ValueError, match="psd_elimination must be 'off' or 'search_free'") as e:
        SA.psd_elimination({"psd_elimination": bad})
    assert repr(str(bad)) in str(e.value)


def test_is_inert_on_plain_templates_and_says_so_once_on_unserved_psd_templates(monkeypatch):
    monkeypatch.setattr(SA, "_WARNED", set())
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # a plain template (no PSD block, variant -1): silent and off, whatever the key says
        assert SA.psd_elimination_active("search_free", -1, False) is False
        assert SA.psd_elimination_active("off", -1, False) is False and SA.psd_elimination_active("off", 1, True) is False and SA.psd_elimination_active("off", -1, True) is False
        assert SA.psd_elimination_active("search_free", 0, True) is True and SA.psd_elimination_active("search_free", 2, True) is True
    with pytest.warns(UserWarning, match="psd_elimination='search_free' is ignored"):
        assert SA.psd_elimination_active("search_free", -1, True) is False
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # once
        assert SA.psd_elimination_active("search_free", -1, True) is False


def test_the_other_keys_are_untouched_by_it():
    args = {"psd_elimination": "search_free", "jvp_mode": "direct", "refine_steps": 2, "newton_first": 1}
    assert SA.jvp_mode(args) == "direct" and SA.refine_steps(args) == 2 and SA.newton_first(args) == 1
    assert SA.jvp_mode({"psd_elimination": "search_free"}) == "lsqr" and SA.refine_steps({"psd_elimination": "search_free"}) == 0

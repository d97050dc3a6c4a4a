"""solver_args of the LPGD backward (interfaces/solver_args.py lpgd_rule): the three modes, lpgd_tau, lpgd_rho; what stays as it was.  No GPU."""
import warnings

import numpy as np
import pytest

from cvxpylayers_amd.interfaces import solver_args as sa


def test_defaults_and_values():
    assert sa.lpgd_rule({}) is None and sa.lpgd_rule({"mode": "lsqr"}) is None and sa.lpgd_rule({"mode": "dense", "lpgd_tau": 0.5}) is None
    assert sa.lpgd_rule({"mode": "lpgd"}) == ("lpgd", 0.1, 0.0)
    assert sa.lpgd_rule({"mode": "lpgd_left", "lpgd_tau": 1e-3}) == ("lpgd_left", 1e-3, 0.0)
    assert sa.lpgd_rule({"mode": "lpgd_right", "lpgd_tau": np.float64(2.0), "lpgd_rho": 1}) == ("lpgd_right", 2.0, 1.0)
    assert all(isinstance(v, float) for v in sa.lpgd_rule({"mode": "lpgd", "lpgd_tau": 1, "lpgd_rho": np.int64(3)})[1:])


@pytest.mark.parametrize("key,bad", [("lpgd_tau", 0), ("lpgd_tau", -0.1), ("lpgd_tau", "0.1"), ("lpgd_tau", None), ("lpgd_tau", True), ("lpgd_tau", float("nan")),
                                     ("lpgd_tau", float("inf")), ("lpgd_rho", -1e-9), ("lpgd_rho", "1"), ("lpgd_rho", [0.0]), ("lpgd_rho", False), ("lpgd_rho", float("nan"))])
def test_bad_values_raise_and_name_the_argument(key, bad):
    for mode in ("lpgd", "lsqr"):          # validated whenever given, whatever the mode
        with pytest.raises(ValueError, match=key):
            sa.lpgd_rule({"mode": mode, key: bad})
    assert sa.lpgd_rule({"mode": "lpgd", "lpgd_rho": 0}) == ("lpgd", 0.1, 0.0)


def test_the_names_are_known_and_the_three_modes_are_no_longer_reported_as_ignored():
    assert {"lpgd_tau", "lpgd_rho", "mode"} <= sa._KNOWN_ARGS
    sa.make_settings({"mode": "lpgd", "lpgd_tau": 0.01, "lpgd_rho": 0.5, "eps": 1e-6})
    with pytest.raises(ValueError, match="unknown solver_args"):
        sa.make_settings({"lpgd_step": 0.1})
    sa._WARNED.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for mode in sa.LPGD_MODES:
            sa.note_ignored_args({"acceleration_lookback": 0, "mode": mode}, explicit_lookback=True)
        assert not w, [str(x.message) for x in w]
        sa.note_ignored_args({"acceleration_lookback": 0, "mode": "bicg"}, explicit_lookback=True)
    assert len(w) == 1 and "bicg" in str(w[0].message) and "ignored" in str(w[0].message)
    sa._WARNED.clear()


def test_adjoint_mode_is_what_it_was():
    assert sa.adjoint_mode({}) == "direct" and sa.adjoint_mode({"mode": "dense"}) == "dense"
    assert sa.adjoint_mode({"mode": "lsqr"}) == "lsqr" and sa.adjoint_mode({"mode": "lsmr"}) == "lsqr" and sa.adjoint_mode({"mode": "bicg"}) == "direct"
    for mode in sa.LPGD_MODES:          # (the LPGD modes answered "direct" before they existed; the plugin asks lpgd_rule first)
        assert sa.adjoint_mode({"mode": mode}) == "direct"
    assert sa.lsqr_rule({"mode": "lpgd"}, 3, 4) == sa.lsqr_rule({}, 3, 4)


def test_lpgd_flags_are_counted_apart_and_reported_under_their_own_causes():
    """the two LPGD status bits (16 a perturbed solve failed, 32 a dy entry was dropped) reach the mailbox as bit 0 of a vector marked lpgd=True: one warning that
    names those causes, none that speaks of a degenerate active set; flags of an ordinary adjoint between the same two forwards keep their own warning and counts"""
    from test_plugin_args import _flags, _mailbox
    box, dev = _mailbox()
    box.note_adjoint_flags(_flags(1, 0, 0, 1), 4, lpgd=True)          # slot 1: two of four
    box.note_adjoint_flags(_flags(0, 2, 0), 3)                        # slot 2: an ordinary adjoint, one of three
    box.note_adjoint_flags(_flags(0, 0), 2, lpgd=True)                # slot 1 again: the LPGD two-of-four are folded first, into their own count
    assert (box.lpgd_count, box.lpgd_total, box.adj_count, box.adj_total) == (2, 4, 0, 0) and box.adj_pending == [(2, 3), (1, 2)]
    box.note_adjoint_flags(_flags(1), 1)                              # slot 2 again, ordinary: the slot is no LPGD slot
    assert (box.lpgd_count, box.lpgd_total, box.adj_count, box.adj_total) == (2, 4, 1, 3) and box.lpgd_slots == {1}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        box.report_flagged_adjoints()
        said = [str(x.message) for x in w]
        assert len(said) == 2, said
        assert any("MI355 adjoint: 2 of 4" in t and "degenerate active" in t for t in said)
        lp = [t for t in said if "MI355 LPGD backward: 2 of 6" in t]
        assert len(lp) == 1 and "perturbed solve failed" in lp[0] and "dropped" in lp[0] and "degenerate" not in lp[0]
        assert (box.lpgd_count, box.lpgd_total, box.adj_count, box.adj_total, box.adj_pending) == (0, 0, 0, 0, [])
        box.note_adjoint_flags(_flags(0, 0, 0), 3, lpgd=True)         # a clean LPGD backward: counted, not reported
        box.report_flagged_adjoints()
        assert len(w) == 2
    assert dev.syncs == []


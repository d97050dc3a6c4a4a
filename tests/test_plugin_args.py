"""Solver arguments the plugin accepts for compatibility with the DIFFCP plugin (diffcp_if.py:356-367) but does not act on are SAID, once per
process and topic, not swallowed: an EXPLICIT acceleration_lookback > 1 (one-pair history), mode other than lsqr / dense, solve_method, n_jobs_*.
The default configuration stays silent (a call that is valid for the reference must survive `-W error`)."""
import warnings

import pytest


def _fresh():
    from cvxpylayers_amd.interfaces import mi355_if
    mi355_if._WARNED.clear()
    return mi355_if


def test_lookback_beyond_one_pair_is_said_once_and_only_when_it_was_asked_for():
    m = _fresh()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m.note_ignored_args({"acceleration_lookback": 10}, explicit_lookback=False)          # SCS's default, forwarded: silent
        assert not w
        m.note_ignored_args({"acceleration_lookback": 10}, explicit_lookback=True)
        m.note_ignored_args({"acceleration_lookback": 5}, explicit_lookback=True)
    assert len(w) == 1 and "ONE-pair" in str(w[0].message) and "SCS's default" not in str(w[0].message)


@pytest.mark.parametrize("lb", [0, 1])
def test_lookback_zero_and_one_are_exactly_what_runs(lb):
    m = _fresh()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m.note_ignored_args({"acceleration_lookback": lb}, explicit_lookback=True)
    assert not w


def test_mode_lsqr_lsmr_and_dense_are_acted_on_other_modes_and_n_jobs_are_reported():
    m = _fresh()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m.note_ignored_args({"acceleration_lookback": 0, "mode": "lsqr", "n_jobs_forward": 4}, explicit_lookback=True)          # mode="lsqr": diffcp's LSQR adjoint (ce_vjp_lsqr)
        m.note_ignored_args({"acceleration_lookback": 0, "mode": "dense", "n_jobs_backward": -1}, explicit_lookback=True)       # mode="dense": the direct elimination
        m.note_ignored_args({"acceleration_lookback": 0, "mode": "lsmr"}, explicit_lookback=True)                               # mode="lsmr": the iterative adjoint under LSMR's recurrences (ce_set_lsqr_variant)
        m.note_ignored_args({"acceleration_lookback": 0, "mode": "bicg"}, explicit_lookback=True)
    msgs = [str(x.message) for x in w]
    assert len(msgs) == 3 and any("'mode'" in t and "bicg" in t for t in msgs) and any("n_jobs_forward" in t for t in msgs) and any("n_jobs_backward" in t for t in msgs)
    assert m.adjoint_mode({"mode": "lsmr"}) == "lsqr" and m.lsqr_rule({"mode": "lsmr"}, 3, 4)[4] == "lsmr" and m.lsqr_rule({"mode": "lsqr"}, 3, 4)[4] == "lsqr"
    assert m.unpack_rule((1e-9, 1e-9, 7), 3, 4) == (1e-9, 1e-9, 7, "full", "lsqr") and m.unpack_rule((1e-9, 1e-9, 7, "reduced"), 3, 4)[3:] == ("reduced", "lsqr") and m.unpack_rule(None, 3, 4)[2] == 16
    assert m.adjoint_mode({"mode": "lsqr"}) == "lsqr" and m.adjoint_mode({"mode": "dense"}) == "dense" and m.adjoint_mode({}) == "direct"      # (default: elimination + device-side LSQR re-solve of rank-deficient instances; "dense": the elimination alone)
    # and they still pass validation (unknown names do not)
    m.make_settings({"mode": "lsqr", "n_jobs_forward": 4, "eps": 1e-6})
    with pytest.raises(ValueError):
        m.make_settings({"lookback": 3})


def test_status_counts_are_recomputed_when_the_device_summary_never_arrives():
    """ensure (outcome_mailbox.OutcomeMailbox; ConeEngine.ensure_summary delegates to it): a ready flag still clear AFTER the stream was drained means the
    device's stores did not reach the pinned buffer; the counts then come from the status vector itself (min, #inaccurate, #flagged) and the engine stops
    spin-polling -- said once."""
    import torch
    m = _fresh()
    box = m.OutcomeMailbox(launch=lambda vec, out: None, synchronize=lambda all_streams=False: None, pin=False)          # a launcher whose stores never arrive
    box.enqueue(torch.tensor([1, 2, 1, -2, 2], dtype=torch.int32), 0)
    box.enqueue(torch.tensor([0, 4, 1, 0], dtype=torch.int32), 2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        box.ensure(0)
        box.ensure(2)
        box.ensure(1)            # nothing enqueued in that slot: left alone
    assert box.slots[0].tolist() == [-2, 2, 5, 1]          # min status, two "solved, inaccurate", five with (v & 3) != 0
    assert box.slots[2].tolist() == [0, 0, 1, 1]           # adjoint flags: bit 2 (rank-deficient, 4) is not a failure, bits 0-1 are
    assert box.slots[1].tolist() == [0, 0, 0, 0]
    assert box.no_spin and len(w) == 1 and "did not arrive" in str(w[0].message)
    box.slots[0] = [1, 0, 0, 1]                            # a slot whose flag IS set is never touched
    box.ensure(0)
    assert box.slots[0].tolist() == [1, 0, 0, 1]


# ---- the reporting rules of the outcome mailbox, driven without a GPU.  The device is a stand-in: launches are recorded and "land" (three counts, then
#      the ready flag, like ce_status_summary writes them) at once, when the test says so, or when the host synchronises.
class _Device:
    def __init__(self, land_at_once):
        self.land_at_once, self.box = land_at_once, None
        self.launches, self.syncs, self.in_flight = [], [], []          # (slot, flagged count folded so far) per launch; "stream" / "device" per synchronisation

    def launch(self, vec, out):
        self.launches.append((self.box.last_slot, self.box.adj_count))
        self.in_flight.append((self.box.last_slot, vec, out))
        if self.land_at_once:
            self.land()

    def land(self, slot=None):
        import torch
        for sl, vec, out in [e for e in self.in_flight if slot in (None, e[0])]:
            v = vec.numpy()
            out[:] = torch.tensor([int(v.min()), int((v == 2).sum()), int(((v & 3) != 0).sum()), 1], dtype=torch.int32)
        self.in_flight = [e for e in self.in_flight if slot not in (None, e[0])]

    def synchronize(self, all_streams=False):
        self.syncs.append("device" if all_streams else "stream")
        self.land()


def _mailbox(land_at_once=True):
    dev = _Device(land_at_once)
    dev.box = _fresh().OutcomeMailbox(dev.launch, dev.synchronize, pin=False)
    return dev.box, dev


def _flags(*v):
    import torch
    return torch.tensor(v, dtype=torch.int32)


def test_backward_calls_alternate_slots_one_and_two_and_a_slot_is_folded_before_it_is_reused():
    box, dev = _mailbox()
    box.note_adjoint_flags(_flags(1, 0, 2, 0, 0), 5)          # two flagged of five -> slot 1
    box.note_adjoint_flags(_flags(0, 1, 0), 3)                # one of three       -> slot 2
    assert box.adj_pending == [(1, 5), (2, 3)] and (box.adj_count, box.adj_total) == (0, 0)
    box.note_adjoint_flags(_flags(0, 0), 2)                   # slot 1 again: its two-of-five are folded BEFORE the launch that overwrites them
    box.note_adjoint_flags(_flags(3, 3, 3, 3), 4)             # slot 2 again
    assert [sl for sl, _ in dev.launches] == [1, 2, 1, 2]
    assert [cnt for _, cnt in dev.launches] == [0, 0, 2, 3]
    assert box.adj_pending == [(1, 2), (2, 4)] and (box.adj_count, box.adj_total) == (3, 8)
    assert dev.syncs == []                                    # every flag was set: nothing to wait for
    box.note_adjoint_flags(_flags(), 0)                       # an empty batch takes no slot
    assert box.adj_seq == 4 and len(dev.launches) == 4


def test_backward_calls_between_two_forwards_give_one_warning_with_summed_counts_and_the_counts_reset():
    box, dev = _mailbox()
    for adj, bs in ((_flags(1, 0, 0), 3), (_flags(0, 2, 1, 0), 4), (_flags(0, 0), 2), (_flags(3), 1)):
        box.note_adjoint_flags(adj, bs)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        box.enqueue(_flags(1, 1, 1), 0)                       # the next forward: its status summary, read, then the report
        assert box.read()[0][:2] == [1, 0]
        box.report_flagged_adjoints()
        assert len(w) == 1 and "MI355 adjoint: 4 of 10 instances of the previous backward pass were flagged" in str(w[0].message)
        assert (box.adj_count, box.adj_total, box.adj_pending) == (0, 0, [])
        box.report_flagged_adjoints()                         # nothing since: silent
        box.note_adjoint_flags(_flags(0, 0, 0), 3)            # a clean backward: counted, not reported
        box.report_flagged_adjoints()
        assert len(w) == 1 and (box.adj_count, box.adj_total, box.adj_pending) == (0, 0, [])
    assert dev.syncs == []


def test_rank_deficient_bit_alone_is_not_a_flagged_adjoint():
    """bit 2 (value 4: rank-deficient system, the reference's LSQR returns a basic solution there too) is no failure; bits 0-1 are.  The counts are taken from
    the flag vectors by the mailbox's own recomputation (stores that never arrive), not by the stand-in."""
    m = _fresh()
    syncs = []
    box = m.OutcomeMailbox(lambda vec, out: None, lambda all_streams=False: syncs.append(all_streams), pin=False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        box.note_adjoint_flags(_flags(4, 4, 0, 12), 4)
        box.report_flagged_adjoints()
        assert [str(x.message) for x in w if "MI355 adjoint" in str(x.message)] == [] and (box.adj_count, box.adj_total) == (0, 0)
        box.note_adjoint_flags(_flags(4, 1, 6, 0, 5), 5)
        box.report_flagged_adjoints()
    said = [str(x.message) for x in w if "MI355 adjoint" in str(x.message)]
    assert len(said) == 1 and "3 of 5 instances" in said[0]
    assert syncs == [True, True]                              # folding a slot whose flag is clear waits for the whole device: the backward may have run on another stream


def test_asynchronous_mode_never_waits_for_a_slot_it_would_reuse():
    box, dev = _mailbox(land_at_once=False)
    box.async_mode = True
    box.note_adjoint_flags(_flags(1, 0), 2)                   # slot 1, still in flight
    box.note_adjoint_flags(_flags(0, 0, 0), 3)                # slot 2, still in flight
    box.note_adjoint_flags(_flags(3, 3, 3, 3), 4)             # would reuse slot 1, whose flag is clear: the sequence number is taken back, nothing is enqueued
    assert box.adj_seq == 2 and len(dev.launches) == 2 and dev.syncs == []
    assert box.adj_pending == [(1, 2), (2, 3)] and (box.adj_count, box.adj_total) == (0, 0)
    dev.land(1)
    box.note_adjoint_flags(_flags(0, 2, 0, 0, 0), 5)          # the same slot once its flag is set: folded, then reused
    assert box.adj_seq == 3 and [sl for sl, _ in dev.launches] == [1, 2, 1] and dev.syncs == []
    assert box.adj_pending == [(2, 3), (1, 5)] and (box.adj_count, box.adj_total) == (1, 2)


def test_non_blocking_report_folds_only_ready_slots_and_is_silent_while_any_is_pending():
    box, dev = _mailbox(land_at_once=False)
    box.async_mode = True
    box.note_adjoint_flags(_flags(1, 1, 0), 3)                # slot 1
    box.note_adjoint_flags(_flags(2, 0), 2)                   # slot 2
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        box.report_flagged_adjoints(block=False)
        assert not w and box.adj_pending == [(1, 3), (2, 2)] and (box.adj_count, box.adj_total) == (0, 0)
        dev.land(1)
        box.report_flagged_adjoints(block=False)              # slot 1 is folded; slot 2 is still out, so nothing is said yet
        assert not w and box.adj_pending == [(2, 2)] and (box.adj_count, box.adj_total) == (2, 3)
        dev.land(2)
        box.report_flagged_adjoints(block=False)
        assert len(w) == 1 and "3 of 5 instances" in str(w[0].message)
        assert (box.adj_count, box.adj_total, box.adj_pending) == (0, 0, [])
    assert dev.syncs == []


def test_previous_asynchronous_forward_is_reported_once_and_only_after_its_flag_is_set():
    box, dev = _mailbox(land_at_once=False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        box.report_previous_async()                           # no asynchronous forward yet, no buffer yet
        box.enqueue(_flags(1, -2, 2, 1, -7, 1, 1), 0)
        box.async_pending = 7
        box.report_previous_async()                           # in flight: silent, still pending
        assert not w and box.async_pending == 7
        dev.land(0)
        box.report_previous_async()
        assert box.async_pending is None and len(w) == 2
        assert "previous forward call (batch of 7) failed (worst status Infeasible/Inaccurate)" in str(w[0].message) and str(w[1].message) == "Solved/Inaccurate."
        box.report_previous_async()                           # said once
        assert len(w) == 2
    assert dev.syncs == []


def test_synchronous_path_synchronises_exactly_when_a_flag_is_clear(monkeypatch):
    box, dev = _mailbox(land_at_once=False)
    box.note_adjoint_flags(_flags(1), 1)                      # slot 1
    box.note_adjoint_flags(_flags(0), 1)                      # slot 2
    dev.land(1)
    box.note_adjoint_flags(_flags(0), 1)                      # reuses slot 1, flag set: no wait
    assert dev.syncs == []
    box.note_adjoint_flags(_flags(2), 1)                      # reuses slot 2, flag clear: the stream is drained first, then the slot folded
    assert dev.syncs == ["stream"] and (box.adj_count, box.adj_total) == (1, 2)
    # a forward: reading polls the ready flag of the last slot enqueued; set -> no synchronisation at all
    dev.land()
    box.enqueue(_flags(1, 2, 1), 0)
    dev.land(0)
    assert box.read()[0] == [1, 1, 3, 1] and dev.syncs == ["stream"]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        box.report_flagged_adjoints()                         # both pending slots are ready: folded without a wait
        assert dev.syncs == ["stream"] and len(w) == 1 and "2 of 4 instances" in str(w[0].message)
        # CE_SPIN_WAIT=0: the stream is synchronised instead of polled, flag clear or not; what it drains has landed, so nothing is recomputed or said
        monkeypatch.setenv("CE_SPIN_WAIT", "0")
        box.enqueue(_flags(1, 1), 0)
        assert box.read()[0] == [1, 0, 2, 1] and dev.syncs == ["stream", "stream"] and not box.no_spin and len(w) == 1
        # a flag still clear when the 0.25 s polling guard runs out: one stream synchronisation
        monkeypatch.delenv("CE_SPIN_WAIT")
        box.enqueue(_flags(-1, 1), 0)
        assert box.read()[0] == [-1, 0, 2, 1] and dev.syncs == ["stream"] * 3 and not box.no_spin and len(w) == 1
        # folding an entry whose flag is clear waits for the whole device (the backward may have run on another stream than the forward just read)
        box.note_adjoint_flags(_flags(0, 1), 2)
        box.report_flagged_adjoints()
        assert dev.syncs == ["stream"] * 3 + ["device"] and "1 of 2 instances" in str(w[-1].message)


@pytest.mark.parametrize("args, plain, with_P", [({}, "per_instance", "per_instance"),
                                                 ({"mode": "lsqr"}, "per_instance_lsqr", "per_instance"),
                                                 ({"mode": "lsmr"}, "per_instance_lsqr", "per_instance"),
                                                 ({"mode": "dense"}, "per_instance_dense", "per_instance_dense")])
def test_adjoint_path_follows_mode_and_the_quadratic_objective(args, plain, with_P):
    """adjoint_path (mi355_if): only the per-instance forward path has a choice; mode "lsqr" / "lsmr" with P inside the kernels is said once and left to the
    direct elimination; the shared-A path keeps its own adjoint whatever the mode."""
    m = _fresh()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert m.adjoint_path("per_instance", False, args) == plain and not w
        assert m.adjoint_path("const_a", False, args) == "const_a" and m.adjoint_path("const_a", True, args) == "const_a" and not w
        assert m.adjoint_path("per_instance", True, args) == with_P
        assert m.adjoint_path("per_instance", True, args) == with_P
    iterative = args.get("mode") in ("lsqr", "lsmr")
    assert len(w) == (1 if iterative else 0) and all("mode='lsqr' is not available with a quadratic objective" in str(x.message) for x in w)


def test_constant_A_is_decided_structurally_from_the_parameter_map():
    """MI355_ctx(reduced_A_mat=...) (the keyword MOREAU_ctx takes; /root/reference moreau_if.py:234-256): the A part of the value vector is batch-invariant
    exactly when no A entry has a parameter column in the map -- decided once at construction, no per-call compare of B x nnzA values and no host sync.
    b may depend on parameters (unlike Moreau's PA_is_constant, which also wants b constant).  Without the map the answer stays None (decided per call)."""
    import numpy as np
    import scipy.sparse as sp
    m = _fresh()
    # 2 x 2 template, CSC of [A | b]: column 0 {rows 0, 1}, column 1 {row 1}, b column {rows 0, 1}  ->  nnz_aug = 5, nnzA = 3
    structure = (np.array([0, 1, 1, 0, 1]), np.array([0, 2, 3, 5]), (2, 3))
    P = 2          # two parameters + the constant column
    only_b = sp.csr_array((np.ones(5), (np.array([0, 1, 2, 3, 4]), np.array([2, 2, 2, 0, 1]))), shape=(5, P + 1))        # A entries constant, b depends on the parameters
    a_too = sp.csr_array((np.ones(5), (np.array([0, 1, 2, 3, 4]), np.array([2, 0, 2, 0, 1]))), shape=(5, P + 1))         # A entry 1 depends on parameter 0
    assert m.MI355_ctx(None, structure, {"z": 0, "l": 2, "q": []}).A_is_constant is None
    assert m.MI355_ctx(None, structure, {"z": 0, "l": 2, "q": []}, reduced_A_mat=only_b).A_is_constant is True
    assert m.MI355_ctx(None, structure, {"z": 0, "l": 2, "q": []}, reduced_A_mat=a_too).A_is_constant is False

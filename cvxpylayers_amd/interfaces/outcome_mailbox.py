"""OutcomeMailbox: how the host learns what the device computed without waiting for it more than once per call.

A pinned (3, 4) int32 buffer the device writes into (ce_status_summary: three counts, then a ready flag):
    slot 0      status of a forward call                     [min status, #Solved/Inaccurate, #with (v & 3) != 0, ready]
    slots 1, 2  adjoint flags of backward calls, alternating [.., .., #flagged (bits 0-1; bit 2 = rank deficient is no failure), ready]
The rules on top of it:
  * a forward reads slot 0 by polling its ready flag (read; CE_SPIN_WAIT=0 or a flag that once failed to arrive: stream synchronisation instead);
  * a backward never waits: its flags are summarised behind the adjoint kernel and reported -- one "N of M" warning -- by the NEXT forward;
  * a slot about to be reused is folded into the running counts first; in asynchronous mode (raise_on_error=False: the host runs ahead of the
    device and must never wait) a slot whose flag is still clear is left alone instead, and that backward's flags go unreported;
  * the non-blocking report folds only slots that are ready and stays silent while any remain pending;
  * the outcome of an asynchronous forward is reported, as warnings, by the first later call that finds its flag set.
The device is reached only through the two callables given at construction, so the rules run on a machine without a GPU (tests/test_plugin_args.py)."""
from __future__ import annotations

import os
import time
import warnings

import torch

from cvxpylayers_amd.interfaces.solver_args import STATUS_NAMES


class OutcomeMailbox:
    def __init__(self, launch, synchronize, pin: bool = True):
        """launch(vec, out): enqueue ce_status_summary of the int32 device vector `vec` into the 4-int host row `out` on the current stream;
        synchronize(all_streams=False): drain the current stream, or the whole device; pin=False: a pageable buffer (no GPU at hand)."""
        self._launch, self._synchronize, self._pin = launch, synchronize, pin
        self.host = None              # the pinned buffer, allocated by the first enqueue
        self.slots = None             # its numpy view (shares the memory)
        self.vec = [None, None, None]           # the device vector behind each slot (ensure can recompute the counts from it)
        self.last_slot = None
        self.no_spin = False          # set once the device's stores failed to arrive: synchronise instead of polling from then on
        self.adj_pending = []         # (slot, batch size) of backward calls not yet folded
        self.adj_seq = 0
        self.adj_count = self.adj_total = 0     # flagged / all instances of the backward calls folded since the last report
        self.lpgd_slots = set()       # the adjoint slots whose pending vector came from an LPGD backward (its causes are others: counted and reported apart)
        self.lpgd_count = self.lpgd_total = 0
        self.async_mode = False       # the most recent forward ran with raise_on_error=False
        self.async_pending = None     # its batch size, until its outcome has been reported

    def enqueue(self, vec: torch.Tensor, slot: int):
        """ce_status_summary of an int32 device vector into pinned slot `slot` (0: status of this forward; 1, 2: adjoint flags of backward calls);
        read with read() once the LAST one enqueued is ready."""
        if self.host is None:
            buf = torch.zeros((3, 4), dtype=torch.int32)
            self.host = buf.pin_memory() if self._pin else buf
            self.slots = self.host.numpy()
        self.slots[slot, 3] = 0                             # "ready" flag, set by the device after the three values
        self.last_slot = slot
        self.vec[slot] = vec                                # (kept for ensure: the counts can be recomputed from the vector if the device's stores never arrive)
        self._launch(vec, self.host[slot])

    def ensure(self, slot: int):
        """Call with the stream drained.  The three counts of a slot are only valid once its ready flag is set; a flag that is still clear AFTER a synchronisation
        means the device's stores did not reach this buffer (a mapping of the pinned buffer that went stale, a box misbehaving): then the counts are recomputed
        from the device vector itself -- correctness does not hang on the fast path -- and the spin-poll is switched off for this engine (every later call would
        otherwise burn its full 0.25 s guard)."""
        arr = self.slots
        if arr[slot, 3] != 0:
            return
        vec = self.vec[slot]
        if vec is None:
            return
        v = vec.detach().to("cpu").numpy()
        arr[slot, 0] = int(v.min()) if v.size else 0
        arr[slot, 1] = int((v == 2).sum()); arr[slot, 2] = int(((v & 3) != 0).sum()); arr[slot, 3] = 1
        if not self.no_spin:
            self.no_spin = True
            warnings.warn("MI355 solver: the status summary written by the device did not arrive in pinned host memory; recomputed from the status vector, "
                          "polling disabled for this engine (stream synchronisation from now on)")

    def read(self):
        """Waits for the summaries enqueued on this stream and returns them.  The last one enqueued carries a ready flag in pinned memory: polling it
        (a few hundred microseconds at most -- the stream holds one solve) spares the wake-up latency of a blocking stream synchronisation, which sits
        in the gap between the forward and the backward kernel of a training step.  CE_SPIN_WAIT=0: always synchronise the stream."""
        slot = self.last_slot
        if slot is not None and os.environ.get("CE_SPIN_WAIT") != "0" and not self.no_spin:
            arr, t0 = self.slots, time.perf_counter()
            while arr[slot, 3] == 0:
                if time.perf_counter() - t0 > 0.25:                 # long solves: hand the core back
                    self._synchronize()
                    self.ensure(slot)
                    break
        else:
            self._synchronize()
            if slot is not None:
                self.ensure(slot)
        return self.slots.tolist()

    def note_adjoint_flags(self, adj, bs, lpgd: bool = False):
        """Called at the END of a backward call: the per-instance flags of the adjoint (more active rows than the direct solve holds, LSQR iteration limit: such
        gradients are zero or inexact) are summarised on the device behind the adjoint kernel -- no host synchronisation on the backward path -- into one of two
        alternating pinned slots.  The NEXT forward call reports them (everything enqueued before its status summary is complete when that is read).  A layer
        applied several times in one graph (the 20 time steps of the supply-chain loop) runs several backward calls between two forwards: the slot a new call is
        about to reuse is folded into the running count first.
        lpgd=True: `adj` comes from an LPGD backward (interfaces/lpgd.py) and holds 1 where a perturbed solve failed or a dual cotangent had no b entry to travel
        in (status bits 16 / 32 brought to bit 0 by the caller: the summary counts bits 0-1); those are counted apart and reported under their own causes."""
        if adj.numel() == 0:
            return
        pend = self.adj_pending
        slot = 1 + (self.adj_seq & 1)
        self.adj_seq += 1
        for k in [k for k, (sl, _) in enumerate(pend) if sl == slot]:          # written two backward calls ago: long complete, but make sure before it is overwritten
            if self.slots is not None and self.slots[slot, 3] == 0:
                if self.async_mode:      # asynchronous forward (raise_on_error=False): the host runs ahead of the device and must never wait -- this call's flags go unreported
                    self.adj_seq -= 1
                    return
                self._synchronize()
            self.fold(pend.pop(k))
        self.enqueue(adj, slot)
        pend.append((slot, bs))
        (self.lpgd_slots.add if lpgd else self.lpgd_slots.discard)(slot)

    def fold(self, entry):
        slot, bs = entry
        # the slot's ready flag, not stream order, says that its three counts have landed: a backward that ran on another stream than the forward whose summary
        # was just read is not ordered by that read
        if self.slots is not None and self.slots[slot, 3] == 0:
            self._synchronize(all_streams=True)
            self.ensure(slot)
        if slot in self.lpgd_slots:
            self.lpgd_count += int(self.slots[slot, 2]); self.lpgd_total += bs
            return
        self.adj_count += int(self.slots[slot, 2])     # bits 0-1; bit 2 (4) = rank-deficient system, basic solution returned like the reference's LSQR does -- not a failure
        self.adj_total += bs

    def report_previous_async(self):
        """raise_on_error=False: the outcome of the PREVIOUS asynchronous forward, if its summary has landed in the pinned slot (never waits)"""
        bs, arr = self.async_pending, self.slots
        if not bs or arr is None or arr[0, 3] == 0:
            return
        self.async_pending = None
        mn, n_inacc = int(arr[0, 0]), int(arr[0, 1])
        if mn < 0:
            warnings.warn(f"MI355 solver: instances of the previous forward call (batch of {bs}) failed (worst status {STATUS_NAMES.get(mn, mn)}); their rows were returned as NaN "
                          "with zero gradients (raise_on_error=False); info['status'] of that call says which")
        if n_inacc:
            warnings.warn("Solved/Inaccurate.")

    def report_flagged_adjoints(self, block: bool = True):
        """forward side: every backward enqueued before this forward's status summary has finished by the time that summary is read
        (block=False -- the asynchronous forward of raise_on_error=False: only the slots whose ready flag is already set are folded)"""
        pend = self.adj_pending
        if not pend and not self.adj_total and not self.lpgd_total:
            return
        if not block:
            ready = [k for k, (sl, _) in enumerate(pend) if self.slots is not None and self.slots[sl, 3] != 0]
            for k in reversed(ready):
                self.fold(pend.pop(k))
            if pend:
                return
        while pend:
            self.fold(pend.pop())
        nbad, bs = self.adj_count, self.adj_total
        self.adj_count = self.adj_total = 0
        if nbad:
            warnings.warn(f"MI355 adjoint: {nbad} of {bs} instances of the previous backward pass were flagged (degenerate active "
                          "set or iteration limit); their gradients are unreliable")
        nbad, bs = self.lpgd_count, self.lpgd_total
        self.lpgd_count = self.lpgd_total = 0
        if nbad:
            warnings.warn(f"MI355 LPGD backward: {nbad} of {bs} instances of the previous backward pass were flagged (a perturbed solve failed: zero gradient; or a "
                          "dual cotangent sat on a row without a b entry and was dropped); info['adjoint']['status'] bits 16 / 32 say which; their gradients are unreliable")

"""MI355 solver plugin: the HIP engine behind cvxpylayers' solver-plugin boundary.

Mirrors the reference DIFFCP plugin  cvxpylayers/interfaces/diffcp_if.py  (same constructor
arguments as DIFFCP_ctx :105-120, same `_CvxpyLayer.apply(P_eval, q_eval, A_eval, cl_ctx,
solver_args, needs_grad, warm_start) -> (primal, dual, aux, data)` convention :329-377 and the same
7-tuple backward :385-403), but every instance is solved and differentiated on the GPU by
csrc/libcone_engine.so through the C ABI in include/cone_engine.h.  No CPU fallback exists.

Not thread-safe (engines are created lazily and cached on MI355_ctx), like moreau_if.py:14-15.

This module holds the context (MI355_ctx) and the autograd function; its parts live next to it and are re-exported here:
solver_args.py (which solver_args exist and what they mean), lpgd.py (the LPGD backward: gradients from perturbed re-solves), newton_first.py (warm-started calls: Newton steps first, the solver for the rest), cone_engine.py (ConeEngine: the ce_handle wrapper), outcome_mailbox.py
(OutcomeMailbox: how forward outcomes and adjoint flags reach the host), quad_epigraph.py (QuadEpigraph), const_a.py (shared-A paths).
"""
from __future__ import annotations

import os
import warnings
from typing import NamedTuple, Optional

import numpy as np
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd.interfaces.cone_engine import ConeEngine
from cvxpylayers_amd.interfaces.lpgd import lpgd_backward
from cvxpylayers_amd.interfaces.newton_first import newton_first_solve, not_served
from cvxpylayers_amd.interfaces.outcome_mailbox import OutcomeMailbox  # noqa: F401  (re-exported, like the names below)
from cvxpylayers_amd.interfaces.quad_epigraph import QuadEpigraph
from cvxpylayers_amd.interfaces.solver_args import (LSQR_ATOL, LSQR_BTOL, STATUS_NAMES, _KNOWN_ARGS, _WARNED, SolverError, _warn_once,  # noqa: F401
                                                    adjoint_mode, dims_to_solver_dict, forward_kernel, jvp_mode, lpgd_rule, lsqr_rule, make_settings, newton_first, note_ignored_args, param_grad, psd_adjoint, psd_elimination, psd_elimination_active, psd_many_active, psd_tangents, qp_adjoint, refine_steps, tri_adjoint, tri_tangents, unpack_rule)


class MI355_ctx:
    """Built once per layer from CVXPY's ParamConeProg; same constructor signature as DIFFCP_ctx
    (diffcp_if.py:105-120): constraint_structure = (indices, indptr, (m, n+1)) is the CSC structure of the
    augmented matrix [A_cvx | b_cvx]."""

    def __init__(self, objective_structure, constraint_structure, dims, lower_bounds=None, upper_bounds=None, options=None, reduced_A_mat=None):
        """reduced_A_mat (optional; the keyword MOREAU_ctx takes, moreau_if.py:159-256): the parameter map of the constraint values, (nnz_aug, P + 1) with the
        constant column last.  When given, whether the A part is batch-invariant is decided HERE, once, from the map's structure -- rows of A entries with no
        parameter column (the reference's PA_is_constant test, moreau_if.py:234-256, restricted to the A rows: b may vary) -- and no call compares values."""
        con_indices, con_ptr, (m, np1) = constraint_structure
        self.A_structure = (np.asarray(con_indices), np.asarray(con_ptr))
        self.A_shape = (int(m), int(np1))
        self.b_idx = np.asarray(con_indices)[con_ptr[-2]:con_ptr[-1]]
        self.dims = dims
        self.cone_dict = dims_to_solver_dict(dims)
        self.options = options or {}
        self.default_device = torch.device("cuda", 0)
        self._engines: dict[int, ConeEngine] = {}
        self.A_is_constant = None          # None: unknown (decided per call from the values, one compare + one host sync); True / False: structural
        if reduced_A_mat is not None:
            nnzA = int(np.asarray(con_ptr)[int(np1) - 1])
            self.A_is_constant = bool(reduced_A_mat[:nnzA, :-1].nnz == 0) if nnzA > 0 else True
        # Quadratic objective 1/2 x^T P x (plugins registered in SUPPORTS_QUAD_OBJ receive P_eval, _quad_form_dpp.py:32,
        # interfaces/__init__.py:35-42): handled as an epigraph SOC block over the Cholesky factor of P (see QuadEpigraph).
        self.quad = QuadEpigraph(objective_structure, self.A_structure, self.A_shape, self.cone_dict) if objective_structure is not None else None
        self._aug_ctx = None

    def augmented(self) -> "MI355_ctx":
        """the cone-program context of the epigraph form (one extra variable, one extra SOC of dimension n + 2)"""
        if self._aug_ctx is None:
            q = self.quad
            self._aug_ctx = MI355_ctx(None, (q.aug_indices, q.aug_indptr, (q.m_aug, q.n + 2)), q.aug_cones, None, None, self.options)
            self._aug_ctx.A_is_constant = False if self.A_is_constant is False else None      # (the Cholesky factor of P enters A: constant only if P is, which the values decide)
            self._aug_ctx.default_device = self.default_device
        return self._aug_ctx

    def engine(self, device: torch.device) -> ConeEngine:
        idx = device.index or 0
        if idx not in self._engines:
            pst = (self.quad.p_indices, self.quad.p_indptr) if self.quad is not None and self.quad.sym_perm is not None else None
            self._engines[idx] = ConeEngine(self.A_structure[0], self.A_structure[1], self.A_shape[1] - 1, self.A_shape[0],
                                            self.cone_dict, torch.device("cuda", idx), p_structure=pst, A_is_constant=self.A_is_constant)
            # A layer is called again and again on related batches (training steps, sweeps): dispatch the instances that ran longest last time first
            # (options={"dispatch_history": False} or CE_DISPATCH_HISTORY=0 switch it off; see include/cone_engine.h)
            self._engines[idx].set_dispatch_history(bool(self.options.get("dispatch_history", True)) and os.environ.get("CE_DISPATCH_HISTORY") != "0")
        return self._engines[idx]


def adjoint_report(info: dict) -> dict:
    """Counts of the last backward through the node that returned `info` (synchronises): instances whose adjoint system was rank deficient, how many of them
    were re-solved by diffcp's LSQR on the device, how many LSQR runs stopped at the iteration limit / were left without gradient."""
    adj = (info.get("adjoint") or {}).get("status")
    if adj is None:
        return dict(rank_deficient=0, lsqr_resolved=0, lsqr_iteration_limit=0, no_gradient=0, backward_ran=False)
    a = adj.detach().cpu().numpy()
    return dict(rank_deficient=int(((a & 4) != 0).sum()), lsqr_resolved=int(((a & 8) != 0).sum()), lsqr_iteration_limit=int(((a & 1) != 0).sum()),
                no_gradient=int(((a & 2) != 0).sum()), backward_ran=True)


def has_tangent(*tensors) -> bool:
    """any of the tensors is a dual tensor of the current torch.autograd.forward_ad level"""
    return any(t is not None and torch.autograd.forward_ad.unpack_dual(t).tangent is not None for t in tensors)


def _detect_batch_size(con_values) -> tuple[int, bool]:
    """diffcp_if.py:34-43"""
    if con_values.dim() == 1:
        return 1, True
    return con_values.shape[1], False


def adjoint_path(path: str, has_P: bool, merged_args: dict) -> str:
    """The path the backward of a node follows, from the path its forward took (ConeEngine.last_path), whether P runs inside the kernels, and solver_args
    `mode` (adjoint_mode).  Only "per_instance" has a choice; mode="lsqr" with a native quadratic objective is said once and left to the direct elimination."""
    if path != "per_instance":
        return path
    mode = adjoint_mode(merged_args)
    if mode == "lsqr" and not has_P:
        return "per_instance_lsqr"          # (the adjoint of this node: diffcp's LSQR instead of the direct elimination)
    if mode == "lsqr":
        _warn_once("lsqr_qp", "MI355 solver: solver_args mode='lsqr' is not available with a quadratic objective inside the kernels; the direct elimination "
                              "differentiates this layer (CE_QP_EPIGRAPH=1 brings the problem to cone form, where mode='lsqr' applies)")
    elif mode == "dense":
        return "per_instance_dense"         # (the elimination alone: no LSQR re-solve of rank-deficient instances)
    return path


def _resolve_warm_start(warm_start, merged_args: dict, batch_size: int, eng: ConeEngine):
    """The initial point of this call as (x, y, s) tensors of (B, .) each, or None for a cold start: the `warm_start` argument of apply() -- True: the
    previous solution of this layer, if it has the same batch size; a triple: used as given -- or, without it, solver_args["warm_starts"]."""
    if warm_start is None and merged_args.get("warm_starts") is not None:
        # diffcp's solve argument (diffcp_if.py:365-367 forwards it): one (x, y, s) triple per instance
        ws = merged_args["warm_starts"]
        if len(ws) != batch_size:
            raise ValueError(f"warm_starts: expected one (x, y, s) triple per instance ({batch_size}), got {len(ws)}")
        warm_start = tuple(torch.stack([torch.as_tensor(np.asarray(t[k]), dtype=torch.float64) for t in ws]) for k in range(3))
    if warm_start is True:                                   # re-use the previous solution of this layer (same batch size)
        prev = eng._last_solution
        return prev if prev is not None and prev[0].shape[0] == batch_size else None
    if warm_start not in (None, False):
        return tuple(t if t.dim() == 2 else t.unsqueeze(0) for t in warm_start)     # (x, y, s) tensors
    return None


class _Saved(NamedTuple):
    """what forward() keeps for backward()"""
    eng: ConeEngine
    A_bm: torch.Tensor
    x: torch.Tensor
    y: torch.Tensor
    s: torch.Tensor
    batch_minor_in: bool                    # A_eval came (nnz_aug, B) contiguous: dA goes back in that layout
    P_bm: Optional[torch.Tensor]            # (B, nnz_p) when P runs inside the kernels
    path: str                               # adjoint_path() of this call
    failed: Optional[torch.Tensor]          # raise_on_error=False: mask of the instances returned as NaN
    lsqr: tuple                             # lsqr_rule() of this call
    q_eval: Optional[torch.Tensor]          # (n+1, B) objective values (linear objective only: ce_jvp_qp and ce_vjp_qp take none)
    jvp_mode: str = "lsqr"                  # jvp_mode() of this call
    ce_settings: Optional[object] = None    # a copy of the ce_settings of this call: the perturbed solves of an LPGD backward run under the same eps, max_iters, acceleration ...
    lpgd: Optional[tuple] = None            # lpgd_rule() of this call: (mode, tau, rho), or None -- the implicit-function adjoint differentiates the node
    fwd_path: str = "per_instance"          # ConeEngine.last_path right after the solve: the path the perturbed solves follow
    qp_adjoint: str = "pivoting"            # qp_adjoint() of this call: "search_free" sends adjoint_many of a native QP node to ce_vjp_qp_many (backward() ignores it)
    tri_adjoint: str = "pivoting"           # tri_adjoint() of this call: "search_free" sends adjoint_many of a node with exponential / power cones to ce_vjp_tri_many (backward() ignores it)
    tri_tangents: str = "loop"              # tri_tangents() of this call: "many" sends tangent_many of a node with exponential / power cones to ce_jvp_tri_many (one-tangent forward-mode AD ignores it)
    psd_ns: bool = False                    # psd_elimination_active() of this call: jvp_mode="direct" runs ce_jvp_psd on this node
    psd_adjoint: bool = False               # psd_many_active(psd_adjoint()) of this call: adjoint_many of a node with PSD blocks runs ce_vjp_psd_many (backward() ignores it)
    psd_tangents: bool = False              # psd_many_active(psd_tangents()) of this call: tangent_many of a node with PSD blocks runs ce_jvp_psd_many (one-tangent forward-mode AD ignores it)


class _ConeLayer(torch.autograd.Function):
    """Same calling convention as diffcp_if._CvxpyLayer (diffcp_if.py:327-403); linear objective (P_eval is None)."""

    @staticmethod
    def forward(P_eval, q_eval, A_eval, cl_ctx, solver_args, needs_grad=True, warm_start=None):
        ctx = cl_ctx.solver_ctx if hasattr(cl_ctx, "solver_ctx") else cl_ctx
        # P_eval given: only for engines that run the quadratic objective inside the kernels (_CvxpyLayer.apply decides)
        batch_size, originally_unbatched = _detect_batch_size(A_eval)
        if originally_unbatched:
            A_eval = A_eval.unsqueeze(1)
            q_eval = q_eval.unsqueeze(1)
        in_device = A_eval.device
        dev = in_device if in_device.type == "cuda" else ctx.default_device
        fwd_kernel = forward_kernel({**ctx.options, **(solver_args or {})})          # (validated before the device is touched)
        if not torch.cuda.is_available():
            raise RuntimeError("MI355 solver needs a ROCm GPU; there is no CPU fallback (use solver='DIFFCP' on CPU)")
        eng = ctx.engine(dev)
        merged_args = {**ctx.options}
        if solver_args:
            merged_args.update(solver_args)
        # SCS runs with Anderson acceleration by default (acceleration_lookback = 10, acceleration_interval = 10) and diffcp forwards
        # SCS's defaults (diffcp_if.py:356-367); ce_default_settings carries the same defaults, so identical solver_args mean the same
        # algorithm here, at the C ABI and in the reference.  The engine keeps a one-pair history whatever the lookback (iteration
        # counts within 2.5 % of lookback 10 on every BASELINE configuration, profiles/r02/aa_memory.json).
        settings = make_settings(merged_args)
        lpgd = lpgd_rule(merged_args)          # (validated here, with the other arguments: a bad lpgd_tau / lpgd_rho raises before anything is enqueued or remembered)
        note_ignored_args({"acceleration_lookback": settings.acceleration_lookback, **{k: merged_args[k] for k in ("mode", "solve_method", "n_jobs_forward", "n_jobs_backward") if k in merged_args}},
                          explicit_lookback="acceleration_lookback" in merged_args)
        n_refine = refine_steps(merged_args)
        qp_adj = qp_adjoint(merged_args)          # (validated with the other arguments; read by adjoint_many alone)
        tri_adj = tri_adjoint(merged_args)        # (likewise)
        param_grad(merged_args)                   # (validated with the other arguments; read by the frontend alone: the plugin boundary has no parameters)
        tri_tan = tri_tangents(merged_args)       # (likewise; read by tangent_many alone)
        n_newton = newton_first(merged_args)
        has_psd = bool(len(eng.cone_dict.get("s", []) or []))
        psd_row = max(eng.psd_ns_variant, eng.psd_tri_ns_variant)          # (at most one is set: triples beside the blocks -> the mixed entries, ConeEngine picks them)
        psd_ns = psd_elimination_active(psd_elimination(merged_args), psd_row, has_psd)
        psd_adj = psd_many_active("psd_adjoint", psd_adjoint(merged_args) == "search_free", psd_row, has_psd)      # (read by adjoint_many alone)
        psd_tan = psd_many_active("psd_tangents", psd_tangents(merged_args) == "many", psd_row, has_psd)          # (read by tangent_many alone)
        warm = _resolve_warm_start(warm_start, merged_args, batch_size, eng)
        box = eng.mailbox
        with torch.cuda.device(dev):
            A_dev = A_eval.detach().to(device=dev, dtype=torch.float64)
            q_dev = q_eval.detach().to(device=dev, dtype=torch.float64)
            batch_minor_in = A_dev.dim() == 2 and A_dev.is_contiguous() and A_dev.shape[1] > 1
            A_bm = eng.to_batch_major(A_dev)
            P_bm = None
            if P_eval is not None:
                if originally_unbatched:
                    P_eval = P_eval.unsqueeze(1)
                P_bm = P_eval.detach().to(device=dev, dtype=torch.float64).t().contiguous()        # (B, nnz_p)
            # solver_args newton_first with a warm start: Newton steps from it, the termination test, and the forward kernels for the instances that miss it
            # (newton_first.py: one 4-byte host read, also under raise_on_error=False); everything below sees the final full-batch result
            # solver_args forward_kernel="wave": one instance per wave where k_fwd_wave serves the template and the solve is per-instance; said once elsewhere
            wave = False
            if fwd_kernel == "wave":
                wave = (P_bm is None and eng.wave_plan()[0] >= 0 and not (n_newton > 0 and warm is not None) and not eng._use_const_a(A_bm))
                if not wave:
                    _warn_once("forward_kernel_none", "MI355 solver: solver_args forward_kernel='wave' is ignored on this template or path: the wave kernel serves a linear "
                                                      "objective, zero / nonnegative / second-order cones, n <= 32, m <= 64 and a per-instance A, and not the remainder "
                                                      "solve of newton_first; the ordinary kernel ran (info['forward']['kernel'] == 'workgroup')")
            nf_info = None
            if n_newton > 0 and warm is not None and batch_size > 0:
                (x, y, s, iters, status, resid), nf_info = newton_first_solve(eng, A_bm, q_dev, settings, warm, n_newton, P_bm=P_bm, psd_ns=psd_ns)
                if nf_info["path"] == "none":
                    _warn_once("newton_first_none", "MI355 solver: solver_args newton_first needs the search-free elimination, which this template or path does not have "
                                                    "(PSD cones, n > 108, a shared A); the ordinary warm-started solve ran (info['newton_first']['path'] == 'none')")
            else:
                x, y, s, iters, status, resid = eng.solve(A_bm, q_dev, settings, warm=warm, P_bm=P_bm, **({"wave": True} if wave else {}))
                if n_newton > 0:
                    nf_info = not_served(n_newton, batch_size)          # (no warm start: nothing to step from, said in info alone)
            path = adjoint_path(eng.last_path, P_bm is not None, merged_args)          # recorded per call: the backward of THIS node must not follow a later solve's path
            # solver_args refine_steps: Newton refinement behind the solve on the same stream, BEFORE the warm-start memory, the saved state and the failure
            # masking are formed: warm starts, backward and jvp all see the refined point.  Failed instances (status < 0) are skipped on the device.
            refine_info = None
            if n_refine > 0:
                refine_info = {"status": None, "steps": None, "resid_before": None, "resid_after": None, "path": "none"}
                if eng.last_path == "per_instance" and status.numel():
                    x, y, s, refine_info = eng.refine(A_bm, q_dev, x, y, s, n_refine, status=status, P_bm=P_bm, psd_ns=psd_ns)
                if refine_info["path"] == "none" and status.numel():
                    _warn_once("refine_none", "MI355 solver: solver_args refine_steps needs the search-free elimination, which this template or path does not have (PSD "
                                              "cones, n > 108, a shared A); the solver's point is returned "
                                              "unrefined (info['refine']['path'] == 'none')")
            eng._last_solution = (x.detach(), y.detach(), s)
            # The reference raises from forward() when an instance fails (diffcp_if.py:365-372), so the host has to learn the outcome here: one tiny
            # reduction kernel + 8 bytes into pinned memory behind the solve (ce_status_summary) and ONE stream synchronisation -- not the status
            # vector through a pageable copy plus host-side reductions.  Per-instance inspection happens only on the failure path.
            raise_on = bool(merged_args.get("raise_on_error", True))
            box.async_mode = not raise_on
            if not raise_on:
                box.report_previous_async()          # (what the previous asynchronous forward left in the pinned slot, if it has landed: warnings only, never a wait)
            if status.numel():
                box.enqueue(status, 0)
            # everything the host can prepare without knowing the outcome happens BEFORE the one synchronisation of this call: the GPU is idle from the
            # end of the solve until the caller's backward reaches it, so host work placed behind the wait is added to that gap
            primal = x.to(in_device)
            dual = y.to(in_device)
            # info["adjoint"] is filled by backward(): "status" = the per-instance bit field of include/cone_engine.h ce_vjp (4: rank-deficient system, 8: gradients
            # are diffcp's LSQR element from the device-side re-solve); adjoint_report(info) counts them
            info = dict(iters=iters, status=status, resid=resid, acceleration=eng.last_acceleration, adjoint={"status": None, "path": path})
            if fwd_kernel == "wave":
                info["forward"] = {"kernel": "k_fwd_wave" if wave else "workgroup"}
            if refine_info is not None:
                info["refine"] = refine_info
            if nf_info is not None:
                info["newton_first"] = nf_info
            lsqr = lsqr_rule(merged_args, eng.n, eng.m)
            fwd_mode = jvp_mode(merged_args)
            if lpgd is not None:
                info["adjoint"].update(path=lpgd[0], tau=lpgd[1], rho=lpgd[2], lpgd_iters=None)
            saved = _Saved(eng, A_bm, x.detach(), y.detach(), s, batch_minor_in, P_bm, path, None, lsqr, q_dev if (P_bm is None or lpgd is not None) else None, fwd_mode,
                           _lib.CeSettings.from_buffer_copy(settings) if lpgd is not None else None, lpgd, eng.last_path, qp_adj, tri_adj, tri_tan, psd_ns, psd_adj, psd_tan) if needs_grad else None
            if status.numel() and not raise_on:
                # raise_on_error=False: the caller has waived the reference's "raise from forward()" contract, so NOTHING forces a host round trip here.  Failed
                # instances are masked ON THE DEVICE (two small elementwise launches, unconditionally), the outcome summary lands in pinned memory behind the
                # solve and is reported -- as warnings -- by the next call that finds it there.  The GPU never waits for the host between the forward and the
                # adjoint kernel (bench.py `async_forward`: the host gap of the step disappears).
                failed = (status < 0)
                nanv = float("nan")
                x = torch.where(failed[:, None], nanv, x); y = torch.where(failed[:, None], nanv, y)
                box.async_pending = batch_size
                if saved is not None:
                    saved = saved._replace(x=x.detach(), y=y.detach(), failed=failed)
                box.report_flagged_adjoints(block=False)
                return x.to(in_device), y.to(in_device), info, (saved, batch_size, originally_unbatched, in_device)
            if status.numel():
                summ = box.read()
                min_status, n_inaccurate = int(summ[0][0]), int(summ[0][1])
                box.report_flagged_adjoints()          # (the flags of the backward calls since the last forward: summarised behind their kernels, complete by now)
            else:
                min_status, n_inaccurate = 1, 0
        any_failed = min_status < 0
        if any_failed and raise_on:
            st = status.cpu()
            bad = int((st < 0).nonzero()[0])
            raise SolverError(f"Solver mi355 returned status {STATUS_NAMES.get(int(st[bad]), int(st[bad]))} "
                              f"for instance {bad} ({int((st < 0).sum())} of {batch_size} instances failed)")
        if n_inaccurate:
            warnings.warn("Solved/Inaccurate.")
        # (raise_on_error=False never reaches this point: its failure masking happens on the device, above)
        # x / y are handed back as `primal` / `dual` (same objects when the input lives on the engine's device), and autograd
        # attaches this node to them: keeping the SAME objects on the node would form a reference cycle (node -> saved ->
        # primal -> grad_fn -> node) that only the cyclic GC breaks, i.e. 167 MB buffers pile up for many steps and the
        # caching allocator falls back to hipMalloc (3 ms each).  Detached aliases share the storage without the cycle.
        return primal, dual, info, (saved, batch_size, originally_unbatched, in_device)

    @staticmethod
    def setup_context(ctx, inputs, outputs):
        _, _, info, backward_data = outputs
        ctx.info = info
        ctx.backward_data = backward_data
        ctx.set_materialize_grads(False)      # an unused output (the duals, most of the time) arrives as None instead of a freshly filled zero tensor: one launch less per step

    @staticmethod
    def jvp(ctx, tP, tq, tA, *_):
        """Forward-mode derivative (torch.autograd.forward_ad; diffcp's `derivative`, which the reference plugin never calls): the tangents of q_eval / A_eval in,
        the tangents of (primal, dual) out, by one launch of the LSQR kernel on M d = -dQ pi (ConeEngine.jvp) under this call's lsqr_rule -- or, with solver_args
        jvp_mode="direct", by the direct elimination with LSQR for the rank-deficient instances only.  A quadratic objective inside the kernels (tP: the tangent
        of P_eval) has the direct elimination alone (ce_jvp_qp: no LSQR behind it; NotImplementedError under the default jvp_mode).  Fills info["jvp"]: status, iters and the path that ran
        ("direct" / "lsqr": a template without the elimination runs LSQR and says so)."""
        saved, batch_size, originally_unbatched, in_device = ctx.backward_data
        if saved is None:
            raise RuntimeError("forward-mode derivative requested from a layer evaluated with needs_grad=False")
        qp = saved.P_bm is not None
        if qp and saved.jvp_mode != "direct":
            raise NotImplementedError("MI355 solver: the LSQR forward-mode derivative is not available with a quadratic objective inside the kernels; "
                                      "pass solver_args jvp_mode='direct' (the elimination with P inside), or set CE_QP_EPIGRAPH=1 to bring the problem "
                                      "to cone form, where the default applies")
        if tq is None and tA is None and (tP is None or not qp):
            return None, None, None, None
        eng, x, y, s, failed = saved.eng, saved.x, saved.y, saved.s, saved.failed
        with torch.cuda.device(eng.device):
            tA_bm = tq_dev = None
            if tA is not None:
                tA_bm = eng.to_batch_major((tA.unsqueeze(1) if originally_unbatched else tA).detach().to(device=eng.device, dtype=torch.float64))
            if tq is not None:
                tq_dev = (tq.unsqueeze(1) if originally_unbatched else tq).detach().to(device=eng.device, dtype=torch.float64)
            if failed is not None:          # masked instances: differentiate at a zero point, return NaN tangents like their NaN primal values
                keep = ~failed[:, None]
                x = torch.where(keep, x, torch.zeros_like(x)); y = torch.where(keep, y, torch.zeros_like(y)); s = torch.where(keep, s, torch.zeros_like(s))
            # a shared-A call whose A values merely coincide may still carry a tangent in A: the shared kernel reads the b entries only
            path = saved.path if (saved.path != "const_a" or tA_bm is None or eng.A_is_constant) else "per_instance"
            if qp:          # tP in the P_eval convention (nnz_p, B), symmetrised like the values by _CvxpyLayer.apply's torch ops
                tP_bm = None
                if tP is not None:
                    tP_bm = (tP.unsqueeze(1) if originally_unbatched else tP).detach().to(device=eng.device, dtype=torch.float64).t().contiguous()
                dx, dy, _, st = eng.jvp(saved.A_bm, x, y, s, tA_bm, tq_dev, method="direct", P_bm=saved.P_bm, tP_bm=tP_bm)
            else:
                dx, dy, _, st = eng.jvp(saved.A_bm, x, y, s, tA_bm, tq_dev, path=path, lsqr=saved.lsqr, q_eval=saved.q_eval, method=saved.jvp_mode, psd_ns=saved.psd_ns)
            if failed is not None:
                nanv = float("nan")
                dx = torch.where(failed[:, None], nanv, dx); dy = torch.where(failed[:, None], nanv, dy)
        if isinstance(ctx.info, dict):
            ctx.info["jvp"] = {"status": st, "iters": eng.last_lsqr_iters, "kernel": eng.last_jvp_kernel, "path": "direct" if eng.last_jvp_kernel in ("ce_jvp", "ce_jvp_qp", "ce_jvp_psd", "ce_jvp_psd_tri") else "lsqr"}
        return dx.to(in_device), dy.to(in_device), None, None

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dprimal, ddual, _info, _data):
        saved, batch_size, originally_unbatched, in_device = ctx.backward_data
        if saved is None:
            raise RuntimeError("backward called on a layer evaluated with needs_grad=False")
        eng, x, y, s, failed = saved.eng, saved.x, saved.y, saved.s, saved.failed
        dP = None
        if dprimal is None and ddual is None:         # nothing flows back through this node
            return None, None, None, None, None, None, None
        with torch.cuda.device(eng.device):
            dx = dprimal.to(device=eng.device, dtype=torch.float64).contiguous() if dprimal is not None else eng.zeros_like_cached(x)
            dy = ddual.to(device=eng.device, dtype=torch.float64).contiguous() if ddual is not None else (None if saved.lpgd is not None else eng.zeros_like_cached(y))
            if failed is not None:          # masked instances: NaN outputs upstream produce NaN cotangents; they contribute nothing
                keep = ~failed[:, None]
                dx = torch.where(keep, dx, torch.zeros_like(dx)); dy = torch.where(keep, dy, torch.zeros_like(dy)) if dy is not None else None
                x = torch.where(keep, x, torch.zeros_like(x)); y = torch.where(keep, y, torch.zeros_like(y)); s = torch.where(keep, s, torch.zeros_like(s))
            lpgd_iters = None
            if saved.lpgd is not None:          # solver_args mode="lpgd" / "lpgd_left" / "lpgd_right": perturbed re-solves instead of an adjoint system (lpgd.py)
                dA, dq, dP_bm, adj, lpgd_iters = lpgd_backward(eng, saved.lpgd, saved.ce_settings, saved.fwd_path, saved.A_bm, saved.q_eval, saved.P_bm, x, y, s, dx, dy,
                                                               failed=failed, batch_minor_out=saved.batch_minor_in)
                dP = dP_bm.t().to(in_device) if dP_bm is not None else None
            elif saved.P_bm is not None:
                dA, dq, adj, dP_bm = eng.vjp(saved.A_bm, x, y, s, dx, dy, batch_minor_out=saved.batch_minor_in, P_bm=saved.P_bm, path=saved.path, lsqr=saved.lsqr)
                dP = dP_bm.t().to(in_device)
            else:
                dA, dq, adj = eng.vjp(saved.A_bm, x, y, s, dx, dy, batch_minor_out=saved.batch_minor_in, path=saved.path, lsqr=saved.lsqr, q_eval=saved.q_eval)
        # (masked instances: zero cotangents at a zero point give exactly zero dA / dq / dP rows from every adjoint kernel -- r = 0 --, no pass over the gradients needed)
        ctx.adj_status = adj
        if isinstance(ctx.info, dict) and isinstance(ctx.info.get("adjoint"), dict):
            ctx.info["adjoint"]["status"] = adj
            if lpgd_iters is not None:
                ctx.info["adjoint"]["lpgd_iters"] = lpgd_iters
        with torch.cuda.device(eng.device):
            if lpgd_iters is None:
                eng.mailbox.note_adjoint_flags(adj, batch_size)
            else:          # (the summary counts bits 0-1 of what it is given: the two LPGD bits -- 16 a perturbed solve failed, 32 a dy entry was dropped -- travel as bit 0, under their own warning)
                eng.mailbox.note_adjoint_flags((adj != 0).to(torch.int32), batch_size, lpgd=True)            # reported by the next forward call (no host sync on the backward path)
        dA = dA.to(in_device)
        dq = dq.to(in_device)
        if originally_unbatched:
            dq = dq.squeeze(1)
            dA = dA.squeeze(1)
            dP = dP.squeeze(1) if dP is not None else None
        return dP, dq, dA, None, None, None, None


def adjoint_many(backward_data, dprimal, ddual, info=None):
    """K cotangents through the node whose forward returned `backward_data` (its fourth output), with no autograd graph: dprimal (K, B, n) and / or ddual (K, B, m),
    either may be None.  Applies what _ConeLayer.backward applies -- device moves, the `failed` mask of a raise_on_error=False call (a zero cotangent at a zero point:
    the caller turns those instances' rows into NaN like their outputs), the saved path / lsqr rule / q_eval, note_adjoint_flags on the OR over the cotangents,
    info["adjoint"]["status"] as (K, B) -- and calls ConeEngine.vjp_many.  Returns dA (K, B, nnz_aug), dq (K, B, n + 1), dP (K, B, nnz_p) or None, all batch-major
    on the engine's device, and the `failed` mask or None."""
    saved, batch_size, _unbatched, _in_device = backward_data
    if saved is None:
        raise RuntimeError("adjoint_many called on a layer evaluated with needs_grad=False")
    if saved.lpgd is not None:
        raise NotImplementedError("MI355 solver: solver_args mode='lpgd' / 'lpgd_left' / 'lpgd_right' has no Jacobian: its gradient is not linear in the cotangent")
    eng, x, y, s, failed = saved.eng, saved.x, saved.y, saved.s, saved.failed
    ref = dprimal if dprimal is not None else ddual
    K = int(ref.shape[0])
    with torch.cuda.device(eng.device):
        f64 = dict(device=eng.device, dtype=torch.float64)
        dx = dprimal.to(**f64).contiguous() if dprimal is not None else torch.zeros((K, batch_size, eng.n), **f64)
        dy = ddual.to(**f64).contiguous() if ddual is not None else None
        if failed is not None:
            keep = ~failed[:, None]
            dx = torch.where(keep, dx, torch.zeros_like(dx)); dy = torch.where(keep, dy, torch.zeros_like(dy)) if dy is not None else None
            x = torch.where(keep, x, torch.zeros_like(x)); y = torch.where(keep, y, torch.zeros_like(y)); s = torch.where(keep, s, torch.zeros_like(s))
        out = eng.vjp_many(saved.A_bm, x, y, s, dx, dy, path=saved.path, lsqr=saved.lsqr, q_eval=saved.q_eval, P_bm=saved.P_bm, qp_many=(saved.qp_adjoint == "search_free"),
                           tri_many=(saved.tri_adjoint == "search_free"), psd_many=saved.psd_adjoint)
        dA, dq, adj = out[:3]
        dP = out[3] if saved.P_bm is not None else None
        if isinstance(info, dict) and isinstance(info.get("adjoint"), dict):
            info["adjoint"]["status"] = adj
            if eng.last_vjp_kernel in ("ce_vjp_qp_many", "ce_vjp_tri_many", "ce_vjp_psd_many", "ce_vjp_psd_tri_many"):
                info["adjoint"]["path"] = eng.last_vjp_kernel
        if K > 0 and batch_size > 0:
            any_k = adj[0].clone()
            for k in range(1, K):
                any_k |= adj[k]
            eng.mailbox.note_adjoint_flags(any_k, batch_size)
    return dA, dq, dP, failed


def param_grad_kind(backward_data):
    """which entry hands the parameter gradient of the node whose forward returned `backward_data` over from the adjoint's factors (solver_args
    param_grad="factors"), or None: "plain" (ce_vjp_many_params / ce_vjp_params: the default adjoint mode on the per-instance path, a linear objective, a template
    with ConeEngine.param_grad_variant >= 0), or -- for MANY cotangents alone, under the rule that sends adjoint_many to the kind's one-factorisation kernel, its own
    key included -- "qp" (a native QP under qp_adjoint="search_free": ce_vjp_qp_many_params), "tri" (exponential / power cones under tri_adjoint="search_free":
    ce_vjp_tri_many_params), "psd" (PSD blocks under psd_adjoint="search_free": ce_vjp_psd_many_params, with triples beside them ce_vjp_psd_tri_many_params)"""
    saved = backward_data[0]
    if saved is None or saved.lpgd is not None or saved.path != "per_instance":
        return None
    eng, L = saved.eng, _lib.lib()
    if saved.P_bm is not None:
        return "qp" if (saved.qp_adjoint == "search_free" and L.ce_vjp_qp_many_variant(eng._h) >= 0) else None
    if saved.q_eval is None:
        return None
    if eng.param_grad_variant >= 0:
        return "plain"
    if saved.tri_adjoint == "search_free" and L.ce_vjp_tri_many_variant(eng._h) >= 0:
        return "tri"
    if saved.psd_adjoint and (L.ce_vjp_psd_many_variant(eng._h) >= 0 or L.ce_vjp_psd_tri_many_variant(eng._h) >= 0):
        return "psd"
    return None


def param_grad_served(backward_data, many: bool = False) -> bool:
    """the node can hand its parameter gradient over from the adjoint's factors: the plain kind always, the QP / TRI / PSD kinds for many cotangents
    (adjoint_many_params) under their own many-cotangent key -- one cotangent belongs to the pivoting kernels there (param_grad_kind)"""
    kind = param_grad_kind(backward_data)
    return kind == "plain" or (many and kind is not None)


def _masked_point(saved, cots):
    """what _ConeLayer.backward does to the point and the cotangents of a raise_on_error=False call: a zero cotangent at a zero point for the masked instances"""
    x, y, s, failed = saved.x, saved.y, saved.s, saved.failed
    if failed is not None:
        keep = ~failed[:, None]
        cots = [None if c is None else torch.where(keep, c, torch.zeros_like(c)) for c in cots]
        x = torch.where(keep, x, torch.zeros_like(x)); y = torch.where(keep, y, torch.zeros_like(y)); s = torch.where(keep, s, torch.zeros_like(s))
    return x, y, s, cots


def adjoint_many_params(backward_data, dprimal, ddual, info, maps, out=None):
    """adjoint_many with the transposed parameter maps applied inside the engine: K cotangents through the node whose forward returned `backward_data`, no dA in
    memory.  maps: the layer's param_grad.ComposedMaps.  Returns g (K, B, Ptot + 1) batch-major on the engine's device -- written into `out` when given --, dq
    (K, B, n + 1) and the `failed` mask or None.  Applies what adjoint_many applies (device moves, the `failed` mask, the saved lsqr rule and q_eval,
    note_adjoint_flags on the OR over the cotangents, info["adjoint"]["status"] as (K, B), info["adjoint"]["path"] == "ce_vjp_many_params") and calls
    ConeEngine.vjp_many_params.  A native QP, exponential / power cones or PSD blocks are served under the node's own many-cotangent key (qp_adjoint / tri_adjoint /
    psd_adjoint = "search_free"): the entry of that kind, named by info["adjoint"]["path"]; the maps of a QP carry its P map.  The node must be served
    (param_grad_served(many=True)): NotImplementedError otherwise, before anything is enqueued."""
    saved, batch_size, _unbatched, _in_device = backward_data
    if saved is None:
        raise RuntimeError("adjoint_many_params called on a layer evaluated with needs_grad=False")
    kind = param_grad_kind(backward_data)
    if kind is None:
        raise NotImplementedError("MI355 solver: this node has no parameter gradient from the adjoint's factors (PSD / exponential / power cones or a quadratic "
                                  "objective without the kind's many-cotangent key, n > 108, a shared A, CE_BWD_NS=0, or a solver_args mode other than the default); use adjoint_many")
    eng = saved.eng
    ref = dprimal if dprimal is not None else ddual
    K = int(ref.shape[0])
    with torch.cuda.device(eng.device):
        f64 = dict(device=eng.device, dtype=torch.float64)
        dx = dprimal.to(**f64).contiguous() if dprimal is not None else torch.zeros((K, batch_size, eng.n), **f64)
        dy = ddual.to(**f64).contiguous() if ddual is not None else None
        x, y, s, (dx, dy) = _masked_point(saved, [dx, dy])
        g, dq, adj = eng.vjp_many_params(saved.A_bm, x, y, s, dx, dy, maps, lsqr=saved.lsqr, q_eval=saved.q_eval, out=out, P_bm=saved.P_bm if kind == "qp" else None,
                                         qp_many=kind == "qp", tri_many=kind == "tri", psd_many=kind == "psd")
        if isinstance(info, dict) and isinstance(info.get("adjoint"), dict):
            info["adjoint"]["status"] = adj
            info["adjoint"]["path"] = eng.last_vjp_kernel
            info["adjoint"]["param_grad"] = "factors"
        if K > 0 and batch_size > 0:
            any_k = adj[0].clone()
            for k in range(1, K):
                any_k |= adj[k]
            eng.mailbox.note_adjoint_flags(any_k, batch_size)
    return g, dq, saved.failed


def adjoint_params(backward_data, dprimal, ddual, info, maps):
    """One cotangent (the .backward() of a layer under param_grad="factors"): dprimal (B, n) and / or ddual (B, m) -> g (B, Ptot + 1) from ConeEngine.vjp_params,
    with what _ConeLayer.backward applies around its vjp call.  None when nothing flows back."""
    saved, batch_size, _unbatched, _in_device = backward_data
    if dprimal is None and ddual is None:
        return None
    eng = saved.eng
    with torch.cuda.device(eng.device):
        f64 = dict(device=eng.device, dtype=torch.float64)
        dx = dprimal.to(**f64).contiguous() if dprimal is not None else eng.zeros_like_cached(saved.x)
        dy = ddual.to(**f64).contiguous() if ddual is not None else eng.zeros_like_cached(saved.y)
        x, y, s, (dx, dy) = _masked_point(saved, [dx, dy])
        g, _dq, adj = eng.vjp_params(saved.A_bm, x, y, s, dx, dy, maps, lsqr=saved.lsqr, q_eval=saved.q_eval)
        if isinstance(info, dict) and isinstance(info.get("adjoint"), dict):
            info["adjoint"]["status"] = adj
        eng.mailbox.note_adjoint_flags(adj, batch_size)
    return g


def tangent_many(backward_data, tP, tq, tA, info=None, method=None, sym_perm=None):
    """K tangents through the node whose forward returned `backward_data`, with no autograd graph -- the forward twin of adjoint_many.  Tangents batch-major in the
    engine's conventions: tA (K, B, nnz_aug), tq (K, B, n + 1), tP (K, B, nnz_p), or (K, .) for one every instance shares; at most two may be None.  Applies what
    _ConeLayer.jvp applies -- device moves, the `failed` mask of a raise_on_error=False call (the derivative at a zero point: the caller turns those instances' rows
    into NaN like their outputs), the saved path / lsqr rule / q_eval, the symmetrisation of tP that _CvxpyLayer.apply gives the values (sym_perm: the permutation,
    None for a one-triangle structure), info["jvp"] with (K, B) status and iterations -- and calls ConeEngine.jvp_many.  method: "direct" / "lsqr", None for the
    call's jvp_mode.  Returns dx (K, B, n), dy (K, B, m) on the engine's device and the `failed` mask or None."""
    saved, batch_size, _unbatched, _in_device = backward_data
    if saved is None:
        raise RuntimeError("tangent_many called on a layer evaluated with needs_grad=False")
    method = saved.jvp_mode if method is None else method
    qp = saved.P_bm is not None
    if qp and method != "direct":
        raise NotImplementedError("MI355 solver: the LSQR forward-mode derivative is not available with a quadratic objective inside the kernels; "
                                  "pass solver_args jvp_mode='direct' (the elimination with P inside), or set CE_QP_EPIGRAPH=1 to bring the problem "
                                  "to cone form, where the default applies")
    eng, x, y, s, failed = saved.eng, saved.x, saved.y, saved.s, saved.failed
    with torch.cuda.device(eng.device):
        f64 = dict(device=eng.device, dtype=torch.float64)
        tA, tq, tP = (None if t is None else t.detach().to(**f64) for t in (tA, tq, tP if qp else None))
        if tP is not None and sym_perm is not None:
            tP = 0.5 * (tP + tP.index_select(tP.dim() - 1, sym_perm.to(eng.device)))
        if failed is not None:
            keep = ~failed[:, None]
            x = torch.where(keep, x, torch.zeros_like(x)); y = torch.where(keep, y, torch.zeros_like(y)); s = torch.where(keep, s, torch.zeros_like(s))
        # a shared-A call whose A values merely coincide may still carry a tangent in A: the shared kernel reads the b entries only
        path = saved.path if (saved.path != "const_a" or tA is None or eng.A_is_constant) else "per_instance"
        if qp:
            dx, dy, _, st = eng.jvp_many(saved.A_bm, x, y, s, tA, tq, method="direct", P_bm=saved.P_bm, tP=tP)
        else:
            dx, dy, _, st = eng.jvp_many(saved.A_bm, x, y, s, tA, tq, path=path, lsqr=saved.lsqr, q_eval=saved.q_eval, method=method, tri_many=(saved.tri_tangents == "many"),
                                         psd_many=saved.psd_tangents)
        if isinstance(info, dict):
            info["jvp"] = {"status": st, "iters": eng.last_lsqr_iters, "kernel": eng.last_jvp_kernel,
                           "path": "direct" if eng.last_jvp_kernel in ("ce_jvp", "ce_jvp_qp", "ce_jvp_many", "ce_jvp_qp_many", "ce_jvp_tri_many", "ce_jvp_psd_many", "ce_jvp_psd_tri", "ce_jvp_psd_tri_many") else "lsqr"}
    return dx, dy, failed


class _CvxpyLayer:
    """What get_torch_cvxpylayer("MI355") returns: `apply(P_eval, q_eval, A_eval, cl_ctx, solver_args, needs_grad, warm_start)
    -> (primal, dual, aux, data)` like every reference plugin (torch/cvxpylayer.py:475-483).  A linear objective goes straight to
    the autograd Function; a quadratic objective (P_eval given, the ctx built with an objective structure) is first brought to
    epigraph cone form by differentiable torch ops (QuadEpigraph), so gradients reach P_eval through autograd."""

    @staticmethod
    def apply(P_eval, q_eval, A_eval, cl_ctx, solver_args=None, needs_grad=True, warm_start=None):
        if not needs_grad and has_tangent(P_eval, q_eval, A_eval):      # forward-mode AD needs what backward() needs
            needs_grad = True
        if P_eval is None:
            return _ConeLayer.apply(None, q_eval, A_eval, cl_ctx, solver_args, needs_grad, warm_start)
        ctx = cl_ctx.solver_ctx if hasattr(cl_ctx, "solver_ctx") else cl_ctx
        if ctx.quad is None:
            raise ValueError("MI355 solver: P_eval was given but the context was built without an objective structure")
        dev0 = A_eval.device if A_eval.device.type == "cuda" else ctx.default_device
        if ctx.quad.sym_perm is not None and os.environ.get("CE_QP_EPIGRAPH") != "1" and ctx.engine(dev0).qp_native:
            # P inside the kernels (SCS 3's QP embedding; plain cones, register-tiled sizes): symmetric values in, dP out
            if not ctx.quad.one_triangle:
                perm = torch.from_numpy(ctx.quad.sym_perm).to(P_eval.device)
                P_eval = 0.5 * (P_eval + P_eval.index_select(0, perm))
            return _ConeLayer.apply(P_eval, q_eval, A_eval, ctx, solver_args, needs_grad, warm_start)
        unbatched = A_eval.dim() == 1
        if unbatched:
            P_eval, q_eval, A_eval = P_eval.unsqueeze(1), q_eval.unsqueeze(1), A_eval.unsqueeze(1)
        if A_eval.device.type != "cuda":
            P_eval, q_eval, A_eval = (t.to(ctx.default_device) for t in (P_eval, q_eval, A_eval))
        q_aug, A_aug = ctx.quad.assemble(P_eval, q_eval, A_eval)
        primal_a, dual_a, info, data = _ConeLayer.apply(None, q_aug, A_aug, ctx.augmented(), solver_args, needs_grad, warm_start)
        primal, dual = ctx.quad.split(primal_a, dual_a)
        return primal, dual, info, data


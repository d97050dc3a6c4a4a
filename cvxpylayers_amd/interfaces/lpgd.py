"""LPGD backward of the MI355 plugin: gradients from perturbed re-solves (Lagrangian proximal gradient descent, Paulus et al. 2024; diffcp's modes "lpgd",
"lpgd_left", "lpgd_right").

For cotangents dx on x*, dy on y*, a step tau > 0 and a proximal weight rho >= 0 the program perturbed at +tau is the forward's own program with
    c+ = c + tau dx - rho x*,   b+ = b - tau dy,   P+ = P + rho I,   A unchanged,
the one at -tau the same with -tau.  With G = dL/dtheta, the envelope gradients of the optimal value (interfaces/optimal_value.py), the gradient is
    lpgd_right: [G(x+, y+) - G(x*, y*)] / tau      lpgd_left: [G(x*, y*) - G(x-, y-)] / tau      lpgd: [G(x+, y+) - G(x-, y-)] / (2 tau).
One backward = per side one ce_lpgd_perturb and one warm-started solve through the dispatcher the forward used (ConeEngine.solve_transient: every template and
path the forward serves, and no trace on the engine), then one ce_lpgd_grad.  Everything is enqueued on the current stream; the per-instance outcomes (zero
cotangent, failed forward, failed perturbed solve, dropped dy entry) are combined on the device.

Facts of the method, not defects: the result is not linear in the cotangent, it depends on tau, and with rho = 0 on a linear program it is a difference of
vertices divided by tau -- informative exactly where the implicit-function adjoint is zero or singular.
"""
from __future__ import annotations

import numpy as np
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd.interfaces.cone_engine import ConeEngine

ST_SOLVE_FAILED = 16          # info["adjoint"]["status"]: a perturbed solve returned a negative status -- the instance's gradient is zero
ST_DY_DROPPED = 32            # a nonzero dy entry sat on a row without a b slot in the template and was dropped


def _has_full_diagonal(eng: ConeEngine) -> bool:
    rows, ptr = eng._p_idx, eng._p_ptr
    return all(j in rows[ptr[j]:ptr[j + 1]] for j in range(eng.n))


def proximal_sibling(eng: ConeEngine) -> ConeEngine:
    """The engine that solves a linear-objective template with the proximal term 1/2 rho |x|^2 in the objective: the same template with a diagonal P structure,
    created on first use and kept beside `eng`.  ValueError when it cannot run P inside the kernels (ce_qp_native() == 0)."""
    sib = getattr(eng, "_lpgd_sibling", None)
    if sib is None:
        diag = (np.arange(eng.n, dtype=np.int32), np.arange(eng.n + 1, dtype=np.int32))
        try:
            sib = ConeEngine(eng._indices, eng._indptr, eng.n, eng.m, eng.cone_dict, eng.device, p_structure=diag, A_is_constant=False)
        except NotImplementedError:          # (a template the library does not build with a P structure at all)
            sib = False
        eng._lpgd_sibling = sib
    if not sib or not sib.qp_native:
        raise ValueError("MI355 solver: lpgd_rho > 0 needs the quadratic term inside the forward kernels, which this template does not have "
                         "(ce_qp_native() == 0: cones beyond zero / nonnegative / second-order, or a size past the register-tiled kernels); pass lpgd_rho=0")
    return sib


def perturbed_points(eng: ConeEngine, rule, settings, path: str, A_bm, q_eval, P_bm, x, y, s, dx, dy):
    """The solutions of the programs perturbed at the sides `rule` asks for: {+1.0 / -1.0: (x_t, y_t)}, the iteration counts per side, the flag word of
    ce_lpgd_perturb and the mask of the instances some perturbed solve failed on (status < 0).  Arguments as lpgd_backward."""
    mode, tau, rho = rule
    st = _lib.CeSettings.from_buffer_copy(settings)
    solver, P_struct = eng, eng.p_structure_dev() if P_bm is not None else None
    if rho > 0.0 and P_bm is not None and not _has_full_diagonal(eng):
        raise ValueError("MI355 solver: lpgd_rho > 0 adds rho to the diagonal of P, but the structure of P does not contain the full diagonal; "
                         "declare the diagonal entries in P's structure or pass lpgd_rho=0")
    if rho > 0.0 and P_bm is None:
        solver = proximal_sibling(eng)
    points, iters, flags, bad = {}, [], None, None
    for sign in ((1.0,) if mode == "lpgd_right" else (-1.0,) if mode == "lpgd_left" else (1.0, -1.0)):
        q_t, A_t, P_t, flags = eng.lpgd_perturb(A_bm, q_eval, x, dx, dy, sign * tau, rho, P_bm=P_bm, p_structure=P_struct)
        if solver is not eng:          # linear objective, rho > 0: the proximal term is the sibling's whole P
            P_t = torch.full((x.shape[0], eng.n), rho, dtype=torch.float64, device=eng.device)
        elif P_bm is not None and P_t is None:
            P_t = P_bm
        xt, yt, _, it, status, _ = solver.solve_transient(A_t if A_t is not None else A_bm, q_t, st, warm=(x, y, s), P_bm=P_t, path=path if solver is eng else None)
        points[sign] = (xt, yt)
        iters.append(it)
        bad = (status < 0) if bad is None else (bad | (status < 0))
    return points, iters, flags, bad


def lpgd_backward(eng: ConeEngine, rule, settings, path: str, A_bm, q_eval, P_bm, x, y, s, dx, dy, failed=None, batch_minor_out: bool = False):
    """The LPGD gradient of one node.  rule = (mode, tau, rho) of solver_args.lpgd_rule; settings: the forward call's ce_settings (a private copy is used); path:
    the path the forward took ("per_instance" / "const_a"); A_bm (B, nnz_aug), q_eval (n+1, B), P_bm (B, nnz_p) or None: the forward's data; (x, y, s): its
    solution; dx (B, n); dy (B, m) or None (no cotangent on the duals: A is not copied); failed (B,) bool or None.
    Returns dA (nnz_aug, B), dq (n+1, B), dP (B, nnz_p) or None, status (B,) int32 (ST_* bits), iters (sides, B) int32."""
    mode, tau, rho = rule
    points, iters, flags, bad = perturbed_points(eng, rule, settings, path, A_bm, q_eval, P_bm, x, y, s, dx, dy)
    skip = ((flags & 1) != 0) | bad
    if failed is not None:
        skip = skip | failed
    a, b, delta = {"lpgd_right": ((x, y), points.get(1.0), tau), "lpgd_left": (points.get(-1.0), (x, y), tau), "lpgd": (points.get(-1.0), points.get(1.0), 2.0 * tau)}[mode]
    dA, dq, dP = eng.lpgd_grad(a[0], a[1], b[0], b[1], delta, skip=skip, batch_minor_A=batch_minor_out, p_structure=eng.p_structure_dev() if P_bm is not None else None)
    status = torch.where(bad, ST_SOLVE_FAILED, 0).to(torch.int32) | torch.where((flags & 2) != 0, ST_DY_DROPPED, 0).to(torch.int32)
    return dA, dq, dP, status, torch.stack(iters)

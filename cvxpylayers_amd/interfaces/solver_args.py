"""Solver-argument rules of the MI355 plugin: which solver_args exist, what they mean for the forward settings and the adjoint, what is said once."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from cvxpylayers_amd import _lib

try:  # subclass diffcp.SolverError when diffcp is importable so `pytest.raises(diffcp.SolverError)` keeps working
    import diffcp as _diffcp  # type: ignore

    _SolverErrorBase = _diffcp.SolverError
except Exception:  # pragma: no cover - diffcp is not installed in this image
    _SolverErrorBase = Exception


class SolverError(_SolverErrorBase):
    """Raised when any instance of the batch is infeasible / unbounded / failed
    (reference contract: tests/test_torch.py:299-316 expects diffcp.SolverError for the whole batch)."""


STATUS_NAMES = {1: "Solved", 2: "Solved/Inaccurate", -1: "Unbounded", -2: "Infeasible", -6: "Unbounded/Inaccurate",
                -7: "Infeasible/Inaccurate", -4: "Failed", 0: "Unfinished"}

_KNOWN_ARGS = {"eps", "eps_abs", "eps_rel", "eps_infeas", "max_iters", "alpha", "rho_x", "scale", "normalize",
               "adaptive_scale", "acceleration_lookback", "acceleration_interval", "verbose", "mode", "solve_method",
               "n_jobs_forward", "n_jobs_backward", "warm_starts", "raise_on_error", "dispatch_history",
               "lsqr_atol", "lsqr_btol", "lsqr_iter_lim", "adjoint_system", "jvp_mode", "refine_steps", "lpgd_tau", "lpgd_rho", "newton_first", "qp_adjoint", "tri_adjoint", "tri_tangents", "psd_elimination", "psd_adjoint", "psd_tangents", "param_grad", "forward_kernel"}

# Stopping rule of the LSQR adjoint (shared-A templates).  diffcp's adjoint (diffcp_if.py:86 -> adj_batch, mode="lsqr") runs LSQR with atol = btol = 1e-8 and an
# iteration limit of 2 N on its N = n + m + 1 operator; the oracle restates exactly that (oracle/cone_oracle.c:85,712).  solver_args may override:
# lsqr_atol / lsqr_btol / lsqr_iter_lim (callers that need gradients to 1e-5 against a direct elimination pass tight values explicitly).
# adjoint_system: "full" (default) = diffcp's (n + m + 1) system M^T r = dz, tau row and column included -- LSQR then returns diffcp's minimum-norm element on
# rank-deficient systems and takes diffcp's number of iterations;  "reduced" = r_tau pinned to 0 (the system of rounds 1-4: the same gradients wherever the
# system is regular and the point accurate, a quarter of the LSQR iterations at loose eps, where the full system is nearly singular AND inconsistent).
LSQR_ATOL, LSQR_BTOL = 1e-8, 1e-8


def lsqr_rule(merged_args: dict, n: int, m: int) -> tuple:
    """(atol, btol, iter_lim, system, method) of the iterative adjoint from merged solver_args; defaults = diffcp's.  method: "lsqr", or "lsmr" for diffcp's mode="lsmr"
    (the same operator and tolerances under Fong & Saunders' LSMR recurrences and stopping tests: ce_set_lsqr_variant)"""
    lim = merged_args.get("lsqr_iter_lim")
    system = str(merged_args.get("adjoint_system", "full"))
    if system not in ("full", "reduced"):
        raise ValueError(f"MI355 solver: adjoint_system must be 'full' or 'reduced', got {system!r}")
    return (float(merged_args.get("lsqr_atol", LSQR_ATOL)), float(merged_args.get("lsqr_btol", LSQR_BTOL)),
            int(lim) if lim not in (None, 0) else 2 * (n + m + 1), system, "lsmr" if str(merged_args.get("mode", "")) == "lsmr" else "lsqr")


def unpack_rule(lsqr, n: int, m: int) -> tuple:
    """(atol, btol, iter_lim, system, method) from a rule of three to five entries (callers of ConeEngine.vjp pass what they care about); None = diffcp's defaults"""
    t = tuple(lsqr) if lsqr is not None else lsqr_rule({}, n, m)
    return t + ("full", "lsqr")[len(t) - 3:] if len(t) < 5 else t[:5]



def adjoint_mode(merged_args: dict) -> str:
    """diffcp's `mode` (adj_batch / solve_and_derivative_batch; diffcp_if.py:86 runs its default "lsqr") for PER-INSTANCE-A templates:
    absent -> "direct": the rank-revealing elimination (k_backward_rt / k_backward: the same gradients as LSQR wherever the adjoint system is regular) and,
    behind it on the device, diffcp's LSQR for exactly the instances the elimination found RANK DEFICIENT (ce_vjp with q_vals; include/cone_engine.h) -- the
    default answer is diffcp's minimum-norm element everywhere, regular instances pay nothing;
    "dense" -> "dense": the elimination alone (a basic solution on rank-deficient systems);
    "lsqr" -> diffcp's LSQR on the full (n + m + 1) system with its stopping rule for every instance (ce_vjp_lsqr).  Shared-A templates run LSQR whatever the mode says."""
    mode = str(merged_args.get("mode", ""))
    return "lsqr" if mode in ("lsqr", "lsmr") else ("dense" if mode == "dense" else "direct")          # ("lsmr": the iterative path with LSMR's recurrences, lsqr_rule()[4])


LPGD_MODES = ("lpgd", "lpgd_left", "lpgd_right")
LPGD_TAU, LPGD_RHO = 0.1, 0.0


def lpgd_rule(merged_args: dict):
    """(mode, tau, rho) of the LPGD backward (interfaces/lpgd.py; Paulus et al. 2024, diffcp's modes of the same names) when solver_args `mode` is "lpgd"
    (central difference), "lpgd_left" or "lpgd_right"; None for every other mode.  lpgd_tau: the perturbation step, a float > 0 (default 0.1); lpgd_rho: the
    proximal weight, a float >= 0 (default 0).  Both are validated whenever they are given, whatever the mode; forward-mode AD ignores them, as diffcp does."""
    mode = merged_args.get("mode")
    if mode not in LPGD_MODES and "lpgd_tau" not in merged_args and "lpgd_rho" not in merged_args:          # (every call of a layer that does not use the feature: nothing to do)
        return None
    vals = {}
    for key, default, ok, what in (("lpgd_tau", LPGD_TAU, lambda v: v > 0.0, "a finite number > 0"), ("lpgd_rho", LPGD_RHO, lambda v: v >= 0.0, "a finite number >= 0")):
        v = merged_args.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(float(v)) or not ok(float(v)):
            raise ValueError(f"MI355 solver: {key} must be {what}, got {v!r}")
        vals[key] = float(v)
    mode = str(merged_args.get("mode", ""))
    return (mode, vals["lpgd_tau"], vals["lpgd_rho"]) if mode in LPGD_MODES else None


def jvp_mode(merged_args: dict) -> str:
    """How the forward-mode derivative (torch.autograd.forward_ad) solves diffcp's M d = -dQ pi on PER-INSTANCE-A templates:
    absent / "lsqr" -> diffcp's LSQR for every instance (ce_jvp_lsqr);
    "direct" -> the search-free elimination the default adjoint runs, and behind it on the device LSQR for exactly the instances it finds rank deficient
    (ce_jvp; exponential / power triples included; PSD blocks under psd_elimination="search_free": ce_jvp_psd).  Templates without that elimination (PSD cones
    by default, n > 108) and shared-A templates run LSQR whatever this says;
    info["jvp"]["path"] tells which one ran.  A quadratic objective inside the kernels has "direct" alone (ce_jvp_qp: the elimination with P inside, no LSQR
    behind it); the default raises NotImplementedError there."""
    mode = str(merged_args.get("jvp_mode", "lsqr"))
    if mode not in ("lsqr", "direct"):
        raise ValueError(f"MI355 solver: jvp_mode must be 'lsqr' or 'direct', got {mode!r}")
    return mode


def qp_adjoint(merged_args: dict) -> str:
    """Which elimination serves MANY cotangents at one solution (CvxpyLayer.jacobian in the reverse direction, interfaces.mi355_if.adjoint_many) when the quadratic
    objective runs inside the kernels:
    absent / "pivoting" -> K calls of ce_vjp_qp, the pivoting kernel, one factorisation per cotangent;
    "search_free" -> one ce_vjp_qp_many call per chunk: the search-free elimination with P inside factors each instance once and returns dA, dq and dP for every
    cotangent (templates without it -- n > 108 -- keep the loop; info["adjoint"]["path"] tells which ran).  The two agree on regular instances; a rank-deficient
    one keeps the search-free route's dropped-variable answer with status 4, hence opt-in.
    The single-cotangent backward of .backward() ignores the key: one cotangent belongs to ce_vjp_qp.  Templates with a linear objective ignore it too."""
    mode = str(merged_args.get("qp_adjoint", "pivoting"))
    if mode not in ("pivoting", "search_free"):
        raise ValueError(f"MI355 solver: qp_adjoint must be 'pivoting' or 'search_free', got {mode!r}")
    return mode


def param_grad(merged_args: dict) -> str:
    """How the parameter gradient of a CvxpyLayer is formed from the adjoint's solution:
    absent / "dA" -> the engine writes dA (nnz_aug entries per instance and cotangent) and dq, and the transposed parameter maps read them back;
    "factors" -> the adjoint kernels keep their small solution (r_x, r_y, r_tau) per (cotangent, instance) pair and one streaming kernel applies the transposed maps
    to the dA entries it evaluates from them: no dA in memory (ce_vjp_many_params behind CvxpyLayer.jacobian(direction="reverse"), ce_vjp_params behind
    .backward(); info["adjoint"]["param_grad"] == "factors").  A parameter with one map entry gets the same bits, the others agree within their terms' rounding.
    Served where ce_param_grad_variant >= 0 on the default adjoint mode (plain cones, a linear objective, n <= 108, per-instance A).  A native quadratic
    objective, exponential / power cones and PSD blocks are served for MANY cotangents (jacobian in the reverse direction) when the layer's own many-cotangent key
    is set beside this one -- qp_adjoint / tri_adjoint / psd_adjoint = "search_free": ce_vjp_qp_many_params / ce_vjp_tri_many_params / ce_vjp_psd_many_params /
    ce_vjp_psd_tri_many_params; one cotangent belongs to the pivoting kernels there.  Every other template or path -- those kinds without their key or with one
    cotangent, mode "dense" / "lsqr" / "lsmr" / the LPGD family, a shared A, CE_BWD_NS=0, forward-mode AD -- ignores the key with one notice and runs the dA
    route.  The plugin boundary (_CvxpyLayer.apply) has no parameters and ignores it."""
    mode = merged_args.get("param_grad", "dA")
    if not isinstance(mode, str) or mode not in ("dA", "factors"):
        raise ValueError(f"MI355 solver: param_grad must be 'dA' or 'factors', got {mode!r}")
    return mode


def tri_adjoint(merged_args: dict) -> str:
    """Which elimination serves MANY cotangents at one solution (CvxpyLayer.jacobian in the reverse direction, interfaces.mi355_if.adjoint_many) on a template with
    exponential / power cones:
    absent / "pivoting" -> K calls of ce_vjp, the pivoting kernel, one factorisation per cotangent;
    "search_free" -> one ce_vjp_tri_many call per chunk: the search-free elimination diagonalises and rotates each triple and factors each instance once for every
    cotangent (templates without it -- PSD cones, n > 108 -- keep the loop; info["adjoint"]["path"] tells which ran).  The two agree on regular instances but need
    not flag the same ones (a pivot search there; here a weighted triple row with 1 - lambda < 1e-5 flags too); a flagged instance gets LSQR's minimum-norm answer,
    hence opt-in.
    The single-cotangent backward of .backward() ignores the key: one cotangent belongs to ce_vjp.  Templates without such cones ignore it too."""
    mode = str(merged_args.get("tri_adjoint", "pivoting"))
    if mode not in ("pivoting", "search_free"):
        raise ValueError(f"MI355 solver: tri_adjoint must be 'pivoting' or 'search_free', got {mode!r}")
    return mode


def tri_tangents(merged_args: dict) -> str:
    """How MANY tangents at one solution (CvxpyLayer.jacobian in the forward direction, interfaces.mi355_if.tangent_many) are served on a template with
    exponential / power cones:
    absent / "loop" -> K calls of ce_jvp: every triple diagonalised, its rows rotated and every instance factored once per tangent;
    "many" -> one ce_jvp_tri_many call per chunk: all of that once per instance for the whole chunk, and one LSQR launch for the flagged instances of every tangent
    (templates without the mode -- PSD cones, n > 108 -- keep the loop; info["jvp"]["kernel"] tells which ran).  Flags and re-solved answers are the loop's.
    Forward-mode AD with one tangent ignores the key: one tangent belongs to ce_jvp.  Templates without such cones ignore it too."""
    mode = str(merged_args.get("tri_tangents", "loop"))
    if mode not in ("loop", "many"):
        raise ValueError(f"MI355 solver: tri_tangents must be 'loop' or 'many', got {mode!r}")
    return mode


def psd_elimination(merged_args: dict) -> str:
    """Whether a per-instance-A template with PSD blocks uses the search-free elimination (ce_jvp_psd, ce_refine_psd: the blocks' rows rotated into the eigenbasis
    of D Pi, then the elimination of the plain cones):
    absent / "off" -> today's routes: forward-mode AD by LSQR whatever jvp_mode says, no refine_steps, no newton_first;
    "search_free" -> jvp_mode="direct" runs ce_jvp_psd (LSQR behind it for the instances it flags), refine_steps and newton_first are served by ce_refine_psd.
    Opt-in: the flagging rule for stiff rows is the triples', not measured on PSD rows.  A template with exponential / power cones beside the blocks is served by
    the mixed entries (ce_jvp_psd_tri, ce_refine_psd_tri) under the same key.  Templates the mode does not serve (no PSD block, a quadratic objective beside
    them, n > 108) ignore the key; psd_elimination_active says so once where the template has a PSD block."""
    mode = str(merged_args.get("psd_elimination", "off"))
    if mode not in ("off", "search_free"):
        raise ValueError(f"MI355 solver: psd_elimination must be 'off' or 'search_free', got {mode!r}")
    return mode


def psd_elimination_active(mode: str, psd_ns_variant: int, has_psd: bool) -> bool:
    """True when this call runs the PSD elimination: the key asks for it and the engine serves the template (ConeEngine.psd_ns_variant >= 0, or
    psd_tri_ns_variant >= 0 where triples stand beside the blocks: the caller passes the one that is set).  A template with a
    PSD block that is not served gets one notice; a template without one is silent (the key is inert there)."""
    if mode != "search_free":
        return False
    if psd_ns_variant >= 0:
        return True
    if has_psd:
        _warn_once("psd_elimination_none", "MI355 solver: solver_args psd_elimination='search_free' is ignored on this template: the search-free elimination does not "
                                           "serve it (a quadratic objective beside the PSD blocks, n > 108, or its footprint exceeds LDS)")
    return False


def psd_adjoint(merged_args: dict) -> str:
    """Which elimination serves MANY cotangents at one solution (CvxpyLayer.jacobian in the reverse direction, interfaces.mi355_if.adjoint_many) on a template with
    PSD blocks:
    absent / "pivoting" -> K calls of ce_vjp, the pivoting kernel: the blocks' Jacobi decompositions and the whole factorisation once per cotangent;
    "search_free" -> one ce_vjp_psd_many call per chunk: the search-free elimination decomposes each block, rotates its rows and factors each instance once for
    every cotangent (info["adjoint"]["path"] tells which ran).  The two agree on regular instances but need not flag the same ones (a pivot search there; here a
    weighted PSD row with 1 - B < 1e-5 flags too -- the triples' rule, carried over, not measured on PSD rows); a flagged instance gets LSQR's minimum-norm answer,
    hence opt-in.
    Independent of psd_elimination, which keeps its documented routes.  The single-cotangent backward of .backward() ignores the key: one cotangent belongs to
    ce_vjp.  With exponential / power cones beside the blocks the one call is ce_vjp_psd_tri_many.  Templates the mode does not serve ignore it: psd_many_active
    says so once where the template has a PSD block."""
    mode = str(merged_args.get("psd_adjoint", "pivoting"))
    if mode not in ("pivoting", "search_free"):
        raise ValueError(f"MI355 solver: psd_adjoint must be 'pivoting' or 'search_free', got {mode!r}")
    return mode


def psd_tangents(merged_args: dict) -> str:
    """How MANY tangents at one solution (CvxpyLayer.jacobian in the forward direction, interfaces.mi355_if.tangent_many) are served on a template with PSD blocks:
    absent / "loop" -> K single-tangent calls (ce_jvp_lsqr on such a template, under psd_elimination="search_free" too);
    "many" -> one ce_jvp_psd_many call per chunk: each block decomposed, its rows rotated and each instance factored once for the whole chunk, and one LSQR launch
    for the flagged instances of every tangent (info["jvp"]["kernel"] tells which ran).  Opt-in: the flagging rule for stiff rows is the triples', carried over.
    Independent of psd_elimination.  Forward-mode AD with one tangent ignores the key.  With exponential / power cones beside the blocks the one call is
    ce_jvp_psd_tri_many.  Templates the mode does not serve ignore it, as psd_adjoint."""
    mode = str(merged_args.get("psd_tangents", "loop"))
    if mode not in ("loop", "many"):
        raise ValueError(f"MI355 solver: psd_tangents must be 'loop' or 'many', got {mode!r}")
    return mode


def psd_many_active(key: str, asked: bool, psd_ns_variant: int, has_psd: bool) -> bool:
    """True when adjoint_many / tangent_many of this call take the many-right-hand-side mode with PSD blocks: `key` (psd_adjoint / psd_tangents) asks for it and
    the engine serves the template (ConeEngine.psd_ns_variant >= 0, or psd_tri_ns_variant >= 0 where triples stand beside the blocks: the modes run on that
    row).  A template with a PSD block that is not served gets one notice
    per key; a template without one is silent (the key is inert there)."""
    if not asked:
        return False
    if psd_ns_variant >= 0:
        return True
    if has_psd:
        _warn_once(key + "_none", f"MI355 solver: solver_args {key} is ignored on this template: the search-free elimination does not serve it (a quadratic objective "
                                  "beside the PSD blocks, n > 108, or its footprint exceeds LDS)")
    return False


def forward_kernel(merged_args: dict) -> str:
    """Which kernel solves the forward problem of a PER-INSTANCE-A template:
    absent / "workgroup" -> the ordinary kernels: one instance per workgroup of 256 or 512 threads (k_fwd2, k_forward_rt, the size-generic kernel);
    "wave" -> k_fwd_wave (ce_solve_wave): one instance per wave, for small templates -- a linear objective, zero / nonnegative / second-order cones, n <= 32,
    m <= 64 (ConeEngine.wave_plan()[0] >= 0).  The same algorithm and settings, so the same statuses, points within the solver's tolerance and iteration counts
    within a check interval; cold solves, warm starts and raise_on_error=False alike.  info["forward"]["kernel"] tells which ran ("k_fwd_wave" / "workgroup").
    Every other template or path -- a quadratic objective, a PSD / exponential / power cone, a larger template, a shared A, the remainder solve of newton_first --
    ignores the key with one notice and runs the ordinary kernel; LPGD's perturbed re-solves always run the ordinary kernel."""
    mode = merged_args.get("forward_kernel", "workgroup")
    if not isinstance(mode, str) or mode not in ("workgroup", "wave"):
        raise ValueError(f"MI355 solver: forward_kernel must be 'workgroup' or 'wave', got {mode!r}")
    return mode


def refine_steps(merged_args: dict) -> int:
    """Newton refinement steps behind the forward solve (ce_refine, ce_refine_qp with a quadratic objective inside the kernels: the search-free elimination on the
    KKT residual, every step safeguarded so that the residual never grows): an integer >= 0, default 0 = none.  Templates without that elimination (PSD
    cones unless psd_elimination="search_free" asks for ce_refine_psd, n > 108, shared-A paths) keep the solver's point and say so once; info["refine"]["path"] tells which."""
    v = merged_args.get("refine_steps", 0)
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
        raise ValueError(f"MI355 solver: refine_steps must be an integer >= 0, got {v!r}")
    return int(v)


def newton_first(merged_args: dict) -> int:
    """Newton steps IN FRONT of the forward solve of a warm-started call (interfaces/newton_first.py: ce_refine / ce_refine_qp from the warm start, then
    ce_check_solved; instances that pass the solver's own termination test are done, the others are solved by the ordinary kernels from the refined point): an
    integer >= 0, default 0 = off.  Acts only with a warm start and where refine_steps acts; info["newton_first"]["path"] tells which."""
    v = merged_args.get("newton_first", 0)
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
        raise ValueError(f"MI355 solver: newton_first must be an integer >= 0, got {v!r}")
    return int(v)


_WARNED: set = set()


def _warn_once(key: str, msg: str):
    """one warning per process and topic (the plugin is called once per training step: repeating it would drown the log)"""
    if key not in _WARNED:
        _WARNED.add(key)
        warnings.warn(msg, stacklevel=3)


def note_ignored_args(merged_args: dict, explicit_lookback: bool):
    """The reference's solver arguments this plugin ACCEPTS but does not act on, said once instead of swallowed silently (diffcp_if.py:356-367 forwards them to
    diffcp / SCS):  acceleration_lookback > 1 -- the kernels keep ONE secant pair whatever the lookback (SCS keeps `lookback` pairs; same fixed point,
    iteration counts within 2.5 % on the BASELINE configurations);  mode other than "lsqr" / "dense" (diffcp's "lsmr") and solve_method -- see adjoint_mode();
    n_jobs_forward / n_jobs_backward -- the batch runs on the GPU."""
    lb = merged_args.get("acceleration_lookback")
    if explicit_lookback and lb is not None and int(lb) > 1:      # (the DEFAULT configuration stays silent -- valid calls must survive `-W error`; info["acceleration"] and the docs carry the one-pair fact)
        _warn_once("lookback", f"MI355 solver: acceleration_lookback={int(lb)}" + ("" if explicit_lookback else " (SCS's default, which the reference forwards)") +
                   " runs as type-I Anderson acceleration with a ONE-pair history (memory 1), not a " + str(int(lb)) + "-pair history; "
                   "pass acceleration_lookback=1 to say so explicitly, 0 to iterate plainly")
    for k in ("mode", "solve_method", "n_jobs_forward", "n_jobs_backward"):
        if k == "mode" and str(merged_args.get(k)) in ("lsqr", "lsmr", "dense") + LPGD_MODES:          # acted on: adjoint_mode(), lpgd_rule()
            continue
        if k in merged_args:
            _warn_once(k, f"MI355 solver: solver_args[{k!r}]={merged_args[k]!r} is accepted for compatibility with the DIFFCP plugin and ignored "
                          "(the adjoint method is fixed per template, the batch is solved on the GPU)")


def dims_to_solver_dict(dims) -> dict:
    """ConeDims (attrs zero/nonneg/soc/exp/psd/p3d) or an SCS-style dict -> {"z","l","q","ep","s","p"}
    (what cvxpy.reductions.solvers.conic_solvers.scs_conif.dims_to_solver_dict returns; diffcp_if.py:8,150)."""
    if isinstance(dims, dict):
        return {"z": int(dims.get("z", dims.get("f", 0))), "l": int(dims.get("l", 0)), "q": [int(v) for v in dims.get("q", [])],
                "ep": int(dims.get("ep", 0)), "s": [int(v) for v in dims.get("s", [])], "p": list(dims.get("p", []))}
    return {"z": int(dims.zero), "l": int(dims.nonneg), "q": [int(v) for v in dims.soc], "ep": int(getattr(dims, "exp", 0)),
            "s": [int(v) for v in getattr(dims, "psd", [])], "p": list(getattr(dims, "p3d", []))}


def make_settings(merged_args: dict) -> _lib.CeSettings:
    """solver_args (SCS / diffcp keyword names) -> ce_settings.  diffcp maps `eps` to eps_abs and eps_rel."""
    unknown = set(merged_args) - _KNOWN_ARGS
    if unknown:
        raise ValueError(f"MI355 solver: unknown solver_args {sorted(unknown)}")
    s = _lib.CeSettings()
    _lib.lib().ce_default_settings(C.byref(s))
    a = dict(merged_args)
    if "eps" in a:
        s.eps_abs = s.eps_rel = float(a["eps"])
    for k in ("eps_abs", "eps_rel", "eps_infeas", "alpha", "rho_x", "scale"):
        if k in a:
            setattr(s, k, float(a[k]))
    for k in ("max_iters", "normalize", "adaptive_scale"):
        if k in a:
            setattr(s, k, int(a[k]))
    # Anderson acceleration: ce_default_settings carries SCS's defaults (lookback 10, interval 10; diffcp forwards them,
    # diffcp_if.py:356-367); acceleration_lookback=0 switches it off.  The kernels keep a one-pair history whatever the lookback.
    if a.get("acceleration_lookback") is not None:
        s.acceleration_lookback = max(int(a["acceleration_lookback"]), 0)
    if a.get("acceleration_interval") not in (0, None):
        s.acceleration_interval = int(a["acceleration_interval"])
    return s

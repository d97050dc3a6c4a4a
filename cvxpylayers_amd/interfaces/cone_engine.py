"""ConeEngine: one ce_handle (one template, one device) behind the C ABI of include/cone_engine.h."""
from __future__ import annotations

import ctypes as C
import os
import warnings
from contextlib import contextmanager
from functools import partial

import numpy as np
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd.interfaces.outcome_mailbox import OutcomeMailbox
from cvxpylayers_amd.interfaces.solver_args import _warn_once, unpack_rule


def _launch_summary(h, device, vec, out):
    """ce_status_summary of `vec` into the pinned 4-int row `out`, on the current stream of `device`"""
    stream = torch.cuda.current_stream(device)
    _lib.check(_lib.lib().ce_status_summary(h, int(vec.numel()), vec.data_ptr(), out.data_ptr(), C.c_void_p(stream.cuda_stream)), "ce_status_summary")


def _synchronize(device, all_streams: bool = False):
    if all_streams:
        torch.cuda.synchronize(device)
    else:
        torch.cuda.current_stream(device).synchronize()


class ConeEngine:
    """Owns one ce_handle (one template, one device)."""

    def __init__(self, indices, indptr, n, m, cone_dict, device: torch.device, p_structure=None, A_is_constant=None):
        self._h = None                    # (first: __del__ runs on a half-built engine too)
        L = _lib.lib()
        self.device = device
        self.A_is_constant = A_is_constant          # structural answer of MI355_ctx (parameter map), when the layer supplied it; None: decided per call from the values
        # what the most recent solve() / vjp() did (introspection: tests, bench, info[...])
        self.last_path = None                 # "per_instance" / "const_a"
        self.last_vjp_many_path = None        # "many" (one ce_vjp_many call) / "loop" (K calls of vjp): what the last vjp_many ran
        self.last_vjp_kernel = None           # "ce_vjp_qp_many" / "ce_vjp_many" / "ce_vjp_tri_many" / "ce_vjp_psd_many" when the last vjp_many made that one call, None when it looped over vjp
        self.last_jvp_many_path = None        # "many" (one ce_jvp_many / ce_jvp_qp_many / ce_jvp_tri_many / ce_jvp_psd_many call) / "loop" (K calls of jvp): what the last jvp_many ran
        self.last_forward_kernel = None       # "k_fwd_wave" when the last solve() ran the one-instance-per-wave kernel (solve(wave=True)), None otherwise
        self.last_acceleration = False        # Anderson acceleration ran
        self.last_const_a_kernel = None       # "k_sa_fwd" / "batch GEMM"
        self.last_lsqr_iters = None           # (B,) int32 iteration counts of the last one-kernel LSQR adjoint / forward derivative
        self.last_jvp_kernel = None           # "ce_jvp" / "ce_jvp_qp" / "ce_jvp_psd" / "ce_jvp_lsqr" / "ce_jvp_shared_a"
        self.dispatch_history = False         # (the library's default; set_dispatch_history)
        self._last_solution = None            # (x, y, s) of the last forward of the layer: warm_start=True
        self._last_q, self._last_q_key = None, None          # objective of the last solve() and the value buffer it belongs to (_recent_q)
        self._aa_warned = False
        self._zero_cache = {}                 # zeros_like_cached
        self._resolve_rule = None             # (atol, btol, iter_lim) last handed to ce_set_adjoint_resolve
        self._ca_cache = None                 # const_a: what is derived from the shared matrix alone (equilibration, row split)
        self.n, self.m = int(n), int(m)
        self._indices = np.ascontiguousarray(indices, dtype=np.int32)
        self._indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        self.nnz_aug = int(self._indptr[-1])
        self.nnzA = int(self._indptr[self.n])
        self.cone_dict = {k: (list(v) if isinstance(v, (list, tuple, np.ndarray)) else v) for k, v in dict(cone_dict).items()}
        q = np.ascontiguousarray(cone_dict.get("q", []), dtype=np.int32)
        s = np.ascontiguousarray(cone_dict.get("s", []), dtype=np.int32)
        t = _lib.CeTemplate()
        t.n, t.m, t.nnz_aug = self.n, self.m, self.nnz_aug
        t.indices = self._indices.ctypes.data_as(C.POINTER(C.c_int))
        t.indptr = self._indptr.ctypes.data_as(C.POINTER(C.c_int))
        t.z, t.l = int(cone_dict.get("z", 0)), int(cone_dict.get("l", 0))
        t.nq, t.q = len(q), q.ctypes.data_as(C.POINTER(C.c_int))
        t.ns, t.s = len(s), s.ctypes.data_as(C.POINTER(C.c_int))
        self._pw = np.ascontiguousarray(cone_dict.get("p", []), dtype=np.float64)
        t.nep, t.np = int(cone_dict.get("ep", 0)), len(self._pw)
        t.p = self._pw.ctypes.data_as(C.POINTER(C.c_double))
        self.nnz_p = 0
        if p_structure is not None:       # quadratic objective: CSC structure of P (n x n)
            self._p_idx = np.ascontiguousarray(p_structure[0], dtype=np.int32)
            self._p_ptr = np.ascontiguousarray(p_structure[1], dtype=np.int32)
            self.nnz_p = int(self._p_ptr[-1])
            t.nnz_p = self.nnz_p
            t.p_indices = self._p_idx.ctypes.data_as(C.POINTER(C.c_int))
            t.p_indptr = self._p_ptr.ctypes.data_as(C.POINTER(C.c_int))
        h = C.c_void_p()
        rc = L.ce_create(C.byref(t), device.index or 0, C.byref(h))
        if rc == -2:
            raise NotImplementedError(L.ce_last_error().decode())
        _lib.check(rc, "ce_create")
        self._h = h
        self.qp_native = bool(self.nnz_p) and bool(L.ce_qp_native(h))     # P runs inside the kernels (else: epigraph form upstream)
        self.psd_tri_ns_variant = int(L.ce_psd_tri_ns_variant(h))         # >= 0: PSD blocks AND triples -- the psd_ns / psd_many flags below call the ce_*_psd_tri* entries on this template
        self.psd_ns_variant = int(L.ce_psd_ns_variant(h))                 # >= 0: ce_jvp_psd / ce_refine_psd serve this template (solver_args psd_elimination)
        a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()          # fixed by ce_create (plan_engine)
        L.ce_get_launch_info(h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        self._launch_info = dict(fwd_lds_bytes=a.value, bwd_lds_bytes=b.value, fwd_mode=c.value, bwd_mode=d.value)
        # outcome reporting (outcome_mailbox.py); bound to the handle and the device, not to self: no reference cycle keeps a dropped engine's buffers alive
        self.mailbox = OutcomeMailbox(partial(_launch_summary, h, device), partial(_synchronize, device))

    def set_dispatch_history(self, on: bool):
        """Longest-first dispatch from the previous call's iteration counts (include/cone_engine.h ce_set_dispatch_history): a scheduling hint, results are
        bit-identical either way."""
        _lib.check(_lib.lib().ce_set_dispatch_history(self._h, int(bool(on))), "ce_set_dispatch_history")
        self.dispatch_history = bool(on)

    def __del__(self):
        try:
            if self._h:
                _lib.lib().ce_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def to_batch_major(self, A_eval: torch.Tensor) -> torch.Tensor:
        """(nnz_aug, B) in any layout -> (B, nnz_aug) contiguous fp64 (zero-copy when it already is)."""
        K, B = A_eval.shape
        if A_eval.dtype != torch.float64:
            A_eval = A_eval.double()
        if B == 0:
            return A_eval.new_empty((0, K))
        if A_eval.stride(0) == 1 and (A_eval.stride(1) == K or B == 1):
            return A_eval.t()
        if not A_eval.is_contiguous():
            A_eval = A_eval.contiguous()
        out = torch.empty((B, K), dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().ce_transpose(self._h, K, B, A_eval.data_ptr(), out.data_ptr(), self._stream()), "ce_transpose")
        return out

    def wave_plan(self):
        """(variant, lds) of the one-instance-per-wave forward kernel k_fwd_wave on this template: the row of csrc/ce_variants_wave.h that serves it (-1: not
        served -- a P structure, a PSD / exponential / power cone, n > 32 or m > 64) and the launch's LDS bytes (0 when not served)."""
        L = _lib.lib()
        return int(L.ce_wave_variant(self._h)), int(L.ce_wave_lds(self._h))

    def solve(self, A_bm: torch.Tensor, q_eval: torch.Tensor, settings, warm=None, P_bm=None, path: str | None = None, wave: bool = False):
        """A_bm (B, nnz_aug) contiguous, q_eval (n+1, B) any strides.  Returns x, y, s, iters, status, resid.
        warm = (x, y, s) of shapes (B, n), (B, m), (B, m): initial point (instances with non-finite entries start cold).
        path: None -- the dispatcher decides (per instance / shared A); "const_a" or "per_instance": the path a caller already knows (solve_transient: the
        perturbed solves of a backward follow their forward's path without comparing values again).
        wave: run ce_solve_wave (k_fwd_wave, one instance per wave; per-instance A, wave_plan()[0] >= 0) instead of ce_solve; an engine it does not serve raises."""
        B = A_bm.shape[0]
        dev = self.device
        if B == 0:        # empty batch: nothing to launch (the C ABI refuses B <= 0)
            f64 = dict(dtype=torch.float64, device=dev)
            self.last_path = "per_instance"
            return (torch.empty((0, self.n), **f64), torch.empty((0, self.m), **f64), torch.empty((0, self.m), **f64),
                    torch.empty((0,), dtype=torch.int32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev), torch.empty((0, 3), **f64))
        if warm is not None:
            if tuple(warm[0].shape) != (B, self.n) or tuple(warm[1].shape) != (B, self.m) or tuple(warm[2].shape) != (B, self.m):
                raise ValueError(f"warm start: expected x {(B, self.n)}, y {(B, self.m)}, s {(B, self.m)}, got "
                                 f"{tuple(warm[0].shape)}, {tuple(warm[1].shape)}, {tuple(warm[2].shape)}")
        if P_bm is not None and not self.qp_native:
            raise RuntimeError("quadratic objective on an engine without native P support (use the epigraph form)")
        # direct engine users (tests, probes): vjp() without q_eval may use the objective of the most recent solve() -- but only for the SAME value buffer
        # (the plugin always passes q_eval explicitly; a q paired with another call's A would silently change the full adjoint system: ADVICE round 5)
        self._last_q, self._last_q_key = q_eval.detach(), (A_bm.data_ptr(), B)
        self.last_forward_kernel = "k_fwd_wave" if wave else None
        if wave and P_bm is not None:
            raise RuntimeError("solve(wave=True): the wave kernel serves a linear objective")
        if not wave and P_bm is None and (path == "const_a" if path is not None else self._use_const_a(A_bm)):
            from cvxpylayers_amd.interfaces.const_a import solve_const_a
            self.last_path = "const_a"
            return solve_const_a(self, A_bm, q_eval, settings, warm=warm)      # (notes itself whether its kernel honours the acceleration)
        self.last_path = "per_instance"
        self._note_acceleration(settings, honoured=wave or bool(_lib.lib().ce_acceleration_available(self._h)), path="size-generic forward kernels")
        if warm is not None:       # the engine reads the initial point from the output buffers (ce_settings.warm_start)
            x, y, s = (t.detach().to(device=dev, dtype=torch.float64).clone().contiguous() for t in warm)
            settings.warm_start = 1
        else:
            x = torch.empty((B, self.n), dtype=torch.float64, device=dev)
            y = torch.empty((B, self.m), dtype=torch.float64, device=dev)
            s = torch.empty((B, self.m), dtype=torch.float64, device=dev)
            settings.warm_start = 0
        iters = torch.empty((B,), dtype=torch.int32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        resid = torch.empty((B, 3), dtype=torch.float64, device=dev)
        if P_bm is not None:
            rc = _lib.lib().ce_solve_qp(self._h, B, A_bm.data_ptr(), 1, self.nnz_aug, q_eval.data_ptr(), q_eval.stride(0),
                                        q_eval.stride(1), P_bm.data_ptr(), C.byref(settings), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                                        iters.data_ptr(), status.data_ptr(), resid.data_ptr(), self._stream())
        elif wave:
            rc = _lib.lib().ce_solve_wave(self._h, B, A_bm.data_ptr(), 1, self.nnz_aug, q_eval.data_ptr(), q_eval.stride(0),
                                          q_eval.stride(1), C.byref(settings), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                                          iters.data_ptr(), status.data_ptr(), resid.data_ptr(), self._stream())
            _lib.check(rc, "ce_solve_wave")
        else:
            rc = _lib.lib().ce_solve(self._h, B, A_bm.data_ptr(), 1, self.nnz_aug, q_eval.data_ptr(), q_eval.stride(0),
                                     q_eval.stride(1), C.byref(settings), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                                     iters.data_ptr(), status.data_ptr(), resid.data_ptr(), self._stream())
        _lib.check(rc, "ce_solve")
        return x, y, s, iters, status, resid

    # what solve() records on the engine about "the most recent solve" (introspection, _recent_q, the one-time acceleration warning)
    # (_aa_warned is NOT among them: the once-per-engine acceleration warning stays said when a perturbed solve was the one to say it)
    _SOLVE_TRACE = ("last_path", "last_forward_kernel", "last_acceleration", "last_const_a_kernel", "_last_q", "_last_q_key")

    def solve_transient(self, A_bm, q_eval, settings, warm=None, P_bm=None, path: str | None = None):
        """solve() that leaves no trace: the handle keeps the retained inputs and the dispatch history of the last ordinary solve (ce_set_transient_solve),
        this object the attributes of _SOLVE_TRACE; _last_solution and the mailbox are not touched by solve() in the first place.  For solves issued from a
        backward pass (interfaces/lpgd.py): a later forward or adjoint of another node sees what it would have seen without them.  A_bm must be contiguous."""
        keep = {k: getattr(self, k) for k in self._SOLVE_TRACE}
        L = _lib.lib()
        _lib.check(L.ce_set_transient_solve(self._h, 1), "ce_set_transient_solve")
        try:
            return self.solve(A_bm, q_eval, settings, warm=warm, P_bm=P_bm, path=path)
        finally:
            L.ce_set_transient_solve(self._h, 0)
            for k, v in keep.items():
                setattr(self, k, v)

    def p_structure_dev(self):
        """(p_rows, p_cols) of this engine's P structure as int32 device tensors in the value order of ce_create (CSC), built once; None without a structure"""
        if not self.nnz_p:
            return None
        if getattr(self, "_p_dev", None) is None:
            cols = np.repeat(np.arange(self.n, dtype=np.int32), np.diff(self._p_ptr))
            self._p_dev = (torch.from_numpy(self._p_idx.copy()).to(self.device), torch.from_numpy(np.ascontiguousarray(cols, dtype=np.int32)).to(self.device))
        return self._p_dev

    def lpgd_perturb(self, A_bm, q_eval, x, dx, dy, tau: float, rho: float, P_bm=None, p_structure=None):
        """The data of the program perturbed by (tau, rho) at the point x with cotangents dx (B, n), dy (B, m) or None (include/cone_engine.h ce_lpgd_perturb).
        Returns q_t (q_eval's shape and strides), A_t (B, nnz_aug) or None when dy is None (solve on A_bm itself), P_t (B, nnz_p) or None when no P_bm is given
        or rho == 0 (use P_bm itself), flags (B,) int32 (bit 0: all-zero cotangent, bit 1: a dy entry without a b slot was dropped).  Enqueues only."""
        B = x.shape[0]
        if B == 0:          # empty batch: nothing to launch (the C ABI refuses B <= 0)
            return (torch.empty_like(q_eval), A_bm.new_empty((0, self.nnz_aug)) if dy is not None else None, None, torch.empty((0,), dtype=torch.int32, device=self.device))
        q_t = torch.empty_strided(tuple(q_eval.shape), tuple(q_eval.stride()), dtype=torch.float64, device=self.device)
        A_t = torch.empty((B, self.nnz_aug), dtype=torch.float64, device=self.device) if dy is not None else None
        pr, pc, nnz_p = self._p_args(p_structure if (P_bm is not None and rho != 0.0) else None)
        P_t = torch.empty((B, nnz_p), dtype=torch.float64, device=self.device) if nnz_p else None
        flags = torch.empty((B,), dtype=torch.int32, device=self.device)
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = _lib.lib().ce_lpgd_perturb(self._h, B, ptr(A_bm) if dy is not None else None, A_bm.stride(0) if dy is not None else 0,
                                        q_eval.data_ptr(), q_eval.stride(0), q_eval.stride(1), ptr(P_bm) if nnz_p else None, pr, pc, nnz_p,
                                        x.data_ptr(), dx.data_ptr(), ptr(dy), float(tau), float(rho), q_t.data_ptr(), ptr(A_t), ptr(P_t), flags.data_ptr(), self._stream())
        _lib.check(rc, "ce_lpgd_perturb")
        return q_t, A_t, P_t, flags

    def lpgd_grad(self, xa, ya, xb, yb, delta: float, skip=None, batch_minor_A: bool = False, p_structure=None):
        """[G(xb, yb) - G(xa, ya)] / delta with G the envelope gradients of value_vjp (ce_lpgd_grad): dA (nnz_aug, B), dq (n+1, B), dP (B, nnz_p) or None.
        batch_minor_A: dA is (nnz_aug, B) contiguous; otherwise the transposed view of a batch-major buffer.  skip (B,) bool / uint8: exact zeros there."""
        B = xa.shape[0]
        f64 = dict(dtype=torch.float64, device=self.device)
        pr, pc, nnz_p = self._p_args(p_structure)
        dA, sA = (torch.empty((self.nnz_aug, B), **f64), (B, 1)) if batch_minor_A else (torch.empty((B, self.nnz_aug), **f64).t(), (1, self.nnz_aug))
        dq = torch.empty((self.n + 1, B), **f64)
        dP = torch.empty((B, nnz_p), **f64) if nnz_p else None
        if B == 0:
            return dA, dq, dP
        sk = skip.view(torch.uint8) if (skip is not None and skip.dtype == torch.bool) else skip
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = _lib.lib().ce_lpgd_grad(self._h, B, xa.data_ptr(), ya.data_ptr(), xb.data_ptr(), yb.data_ptr(), float(delta), ptr(sk),
                                     dA.data_ptr(), *sA, dq.data_ptr(), B, 1, ptr(dP), pr, pc, nnz_p, self._stream())
        _lib.check(rc, "ce_lpgd_grad")
        return dA, dq, dP

    def _recent_q(self, A_bm):
        return self._last_q if (self._last_q is not None and self._last_q_key == (A_bm.data_ptr(), A_bm.shape[0])) else None

    def zeros_like_cached(self, t: torch.Tensor) -> torch.Tensor:
        """A read-only zero tensor of t's shape on this engine's device, allocated once per shape (the cotangent of an output the loss does not use)."""
        cache = self._zero_cache
        key = tuple(t.shape)
        z = cache.get(key)
        if z is None:
            if len(cache) > 8:
                cache.clear()
            z = cache[key] = torch.zeros(key, dtype=torch.float64, device=self.device)
        return z

    # outcome reporting: delegates to the mailbox (kept for direct engine users)
    def enqueue_summary(self, vec: torch.Tensor, slot: int):
        self.mailbox.enqueue(vec, slot)

    def ensure_summary(self, slot: int):
        self.mailbox.ensure(slot)

    def read_summaries(self):
        return self.mailbox.read()

    def status_summary(self, status: torch.Tensor) -> tuple[int, int]:
        """(min status, number of Solved/Inaccurate) of a status vector on this engine's device: one launch + a 12-byte pinned copy + one stream sync."""
        if status.numel() == 0:
            return 1, 0
        with torch.cuda.device(self.device):
            self.mailbox.enqueue(status, 0)
            r = self.mailbox.read()
        return int(r[0][0]), int(r[0][1])

    def _note_acceleration(self, settings, honoured: bool, path: str):
        """Records whether this solve ran with Anderson acceleration (`last_acceleration`, surfaced as info["acceleration"]) and warns
        ONCE per engine when a positive acceleration_lookback -- explicit or the SCS default -- is not honoured by the selected path."""
        self.last_acceleration = bool(settings.acceleration_lookback > 0 and honoured)
        if settings.acceleration_lookback > 0 and not honoured and not self._aa_warned:
            self._aa_warned = True
            warnings.warn(f"MI355 solver: acceleration_lookback={settings.acceleration_lookback} is not implemented on the {path}; "
                          "iterating without Anderson acceleration (pass acceleration_lookback=0 to silence this)")

    def _use_const_a(self, A_bm) -> bool:
        """The batch-GEMM path pays off when the instance is too large for the register / LDS-resident kernels (those are
        faster for small instances even when A is shared).  CE_CONST_A=1 forces it whenever A is batch-invariant, =0 disables it."""
        from cvxpylayers_amd.interfaces.const_a import is_constant_A
        env = os.environ.get("CE_CONST_A")
        if env == "0" or A_bm.shape[0] < 2:
            return False
        if env != "1" and self._launch_info["fwd_mode"] not in (1, 2):
            return False
        if self.A_is_constant is not None:
            return bool(self.A_is_constant)
        return is_constant_A(A_bm, self.nnzA)

    def vjp(self, A_bm, x, y, s, dx, dy, batch_minor_out: bool = False, P_bm=None, path: str | None = None, lsqr: tuple | None = None, q_eval=None):
        """Returns dA (nnz_aug, B), dq (n+1, B), adj_status (B,).  dA is a transposed view of a batch-major buffer (the
        engine-native layout, no extra pass) unless batch_minor_out: then it is (nnz_aug, B) contiguous -- the layout of a
        reference-style A_eval, so that autograd can accumulate it into the leaf without a strided copy (one engine layout pass).
        path: the path ("per_instance" / "const_a") of the forward call being differentiated, as recorded by the caller right
        after solve() -- the autograd node keeps it, so interleaved forward calls of one layer cannot redirect a pending backward.
        None (direct engine users with one solve in flight): the path of the most recent solve().
        lsqr: (atol, btol, iter_lim[, system]) of the shared-A LSQR adjoint (lsqr_rule); None = diffcp's 1e-8 / 1e-8 / 2 (n + m + 1) on the full system.  Ignored by the direct eliminations.
        q_eval: the forward call's (n+1, B) objective values; the shared-A LSQR adjoint then solves diffcp's full (n + m + 1) system (const_a.vjp_const_a)."""
        B = A_bm.shape[0]
        dev = self.device
        if B == 0:
            return (torch.empty((self.nnz_aug, 0), dtype=torch.float64, device=dev), torch.empty((self.n + 1, 0), dtype=torch.float64, device=dev),
                    torch.empty((0,), dtype=torch.int32, device=dev))
        if path is None:
            path = self.last_path
        if path == "const_a" and (self._launch_info["bwd_mode"] in (1, 2) or os.environ.get("CE_CONST_A") == "1"):
            from cvxpylayers_amd.interfaces.const_a import vjp_const_a      # shared A: batched LSQR with GEMMs over the batch
            if q_eval is None:          # direct engine users: the objective of the most recent solve() of this very value buffer, else the reduced system
                q_eval = self._recent_q(A_bm)
            atol, btol, lim, system, method = unpack_rule(lsqr, self.n, self.m)
            if system == "reduced":
                q_eval = None
            with self._lsqr_variant(method):
                return vjp_const_a(self, A_bm, x, y, s, dx, dy, batch_minor_out=batch_minor_out, atol=atol, btol=btol, iter_lim=lim, q_eval=q_eval)
        if path == "per_instance_lsqr":      # solver_args mode="lsqr" on a per-instance-A template: diffcp's LSQR instead of the direct elimination
            if P_bm is not None:
                raise ValueError("MI355 solver: mode='lsqr' is not available with a quadratic objective inside the kernels (CE_QP_EPIGRAPH=1 brings the problem to cone form)")
            atol, btol, lim, system, method = unpack_rule(lsqr, self.n, self.m)
            if q_eval is None and system != "reduced":
                q_eval = self._recent_q(A_bm)
            with self._lsqr_variant(method):
                out = self._vjp_lsqr(A_bm, x, y, s, dx, dy, batch_minor_out, atol, btol, lim, None if system == "reduced" else q_eval)
            if out is not None:
                return out
            path = "per_instance"          # (the LSQR vectors of one instance exceed LDS: warned once, the direct elimination + re-solve serves the call)
        dq = torch.empty((self.n + 1, B), dtype=torch.float64, device=dev)
        adj = torch.empty((B,), dtype=torch.int32, device=dev)
        # rank-deficient instances are re-solved on the device by diffcp's LSQR when the call's q_eval is at hand (ce_vjp); path "per_instance_dense" (solver_args
        # mode="dense") keeps the elimination's basic solution
        resolve = P_bm is None and q_eval is not None and path != "per_instance_dense"          # (q_eval must be given explicitly here: without it, the elimination alone)
        qd, q_args = self._q_args(q_eval if resolve else None)
        if resolve:
            rule = unpack_rule(lsqr, self.n, self.m)[:4]
            if rule[:3] != self._resolve_rule:
                _lib.check(_lib.lib().ce_set_adjoint_resolve(self._h, 1, float(rule[0]), float(rule[1]), 1e8, int(rule[2])), "ce_set_adjoint_resolve")
                self._resolve_rule = rule[:3]
        if batch_minor_out:
            dA = torch.empty((self.nnz_aug, B), dtype=torch.float64, device=dev)
            sk, sb = B, 1
        else:
            dA = torch.empty((B, self.nnz_aug), dtype=torch.float64, device=dev)
            sk, sb = 1, self.nnz_aug
        if P_bm is not None:      # quadratic objective: also dP (B, nnz_p) batch-major
            dP = torch.empty((B, self.nnz_p), dtype=torch.float64, device=dev)
            rc = _lib.lib().ce_vjp_qp(self._h, B, A_bm.data_ptr(), 1, self.nnz_aug, P_bm.data_ptr(), x.data_ptr(), y.data_ptr(),
                                      s.data_ptr(), dx.data_ptr(), dy.data_ptr(), dA.data_ptr(), sk, sb,
                                      dq.data_ptr(), B, 1, dP.data_ptr(), adj.data_ptr(), self._stream())
            _lib.check(rc, "ce_vjp_qp")
            return (dA if batch_minor_out else dA.t()), dq, adj, dP
        rc = _lib.lib().ce_vjp(self._h, B, A_bm.data_ptr(), 1, self.nnz_aug, *q_args, x.data_ptr(), y.data_ptr(),
                               s.data_ptr(), dx.data_ptr(), dy.data_ptr(), dA.data_ptr(), sk, sb,
                               dq.data_ptr(), B, 1, adj.data_ptr(), self._stream())
        _lib.check(rc, "ce_vjp")
        return (dA if batch_minor_out else dA.t()), dq, adj

    def vjp_many(self, A_bm, x, y, s, dx, dy, path: str | None = None, lsqr: tuple | None = None, q_eval=None, P_bm=None, force_loop: bool = False,
                 qp_many: bool = False, tri_many: bool = False, psd_many: bool = False):
        """K cotangents at one solution: dx (K, B, n), dy (K, B, m) or None (zero).  Returns dA (K, B, nnz_aug), dq (K, B, n+1), adj (K, B) -- and dP (K, B, nnz_p) when
        P_bm is given -- all batch-major.  For every k the result is what vjp returns for (dx[k], dy[k]).
        One ce_vjp_many call (each instance factored once, last_vjp_many_path == "many") under the rule that sends vjp to the search-free elimination: path
        "per_instance", q_eval given, no P, and a template with the mode (ce_vjp_many_variant >= 0).  Every other case -- the dense / LSQR / shared-A paths, a quadratic
        objective inside the kernels, templates without the mode, force_loop -- is K calls of vjp, stacked ("loop"): the method is total, and the loop is the comparator.
        qp_many (opt-in, default False): with P_bm, path "per_instance" and ce_vjp_qp_many_variant >= 0, one ce_vjp_qp_many call instead of the K ce_vjp_qp calls
        (last_vjp_many_path == "many", last_vjp_kernel == "ce_vjp_qp_many"): the search-free elimination with P factors each instance once and returns dP as well.
        The two routes agree on regular instances; a rank-deficient one keeps the search-free route's dropped-variable answer with status 4 (no re-solve has a P
        term), where the pivoting kernel of ce_vjp_qp returns its own basic solution -- hence opt-in.  Without P_bm, or on any other path, the flag changes nothing.
        tri_many (opt-in, default False): on a template with exponential / power triples (ce_vjp_tri_many_variant >= 0), path "per_instance", q_eval given, no P, one
        ce_vjp_tri_many call instead of the K ce_vjp calls of the pivoting kernel (last_vjp_many_path == "many", last_vjp_kernel == "ce_vjp_tri_many"): the
        search-free elimination diagonalises and rotates each triple once per instance.  The two kernels agree on regular instances but need not flag the same ones
        (a pivot search there, the stiff-row rule here; a flagged instance gets LSQR's minimum-norm answer) -- hence opt-in.  In every other case the flag changes nothing.
        psd_many (opt-in, default False): on a template with PSD blocks (ce_vjp_psd_many_variant >= 0), under tri_many's conditions, one ce_vjp_psd_many call instead
        of the K ce_vjp calls of the pivoting kernel (last_vjp_kernel == "ce_vjp_psd_many"): each block is decomposed and its rows rotated once per instance.  The
        same caveat on flags (the stiff-row rule, carried over to PSD rows); in every other case the flag changes nothing.  On a template with PSD blocks AND
        triples (ce_vjp_psd_tri_many_variant >= 0) the flag makes the one call ce_vjp_psd_tri_many (last_vjp_kernel names it)."""
        dev = self.device
        f64 = dict(dtype=torch.float64, device=dev)
        K, B = int(dx.shape[0]), int(A_bm.shape[0])
        if path is None:
            path = self.last_path
        many = (not force_loop and path == "per_instance" and q_eval is not None and P_bm is None and _lib.lib().ce_vjp_many_variant(self._h) >= 0)
        many_qp = (not force_loop and qp_many and P_bm is not None and path == "per_instance" and _lib.lib().ce_vjp_qp_many_variant(self._h) >= 0)
        many_tri = (not force_loop and tri_many and not many and path == "per_instance" and q_eval is not None and P_bm is None
                    and _lib.lib().ce_vjp_tri_many_variant(self._h) >= 0)
        many_psd = (not force_loop and psd_many and not many and not many_tri and path == "per_instance" and q_eval is not None and P_bm is None
                    and (_lib.lib().ce_vjp_psd_many_variant(self._h) >= 0 or _lib.lib().ce_vjp_psd_tri_many_variant(self._h) >= 0))
        mixed = many_psd and _lib.lib().ce_vjp_psd_tri_many_variant(self._h) >= 0          # (PSD blocks and triples: the mixed entry, the same arguments)
        self.last_vjp_many_path = "many" if (many or many_qp or many_tri or many_psd) else "loop"
        self.last_vjp_kernel = ("ce_vjp_qp_many" if many_qp else ("ce_vjp_many" if many else ("ce_vjp_tri_many" if many_tri else
                                                                                             (("ce_vjp_psd_tri_many" if mixed else "ce_vjp_psd_many") if many_psd else None))))
        if B == 0 or K == 0:
            out = (torch.empty((K, B, self.nnz_aug), **f64), torch.empty((K, B, self.n + 1), **f64), torch.empty((K, B), dtype=torch.int32, device=dev))
            return out + ((torch.empty((K, B, self.nnz_p), **f64),) if P_bm is not None else ())
        dx = dx.to(**f64).contiguous()
        dy = None if dy is None else dy.to(**f64).contiguous()
        if many_qp:
            A_c = A_bm if (A_bm.stride(1) == 1 and (B == 1 or A_bm.stride(0) == self.nnz_aug)) else A_bm.contiguous()
            xc, yc, sc_, P_c = (t.detach().to(**f64).contiguous() for t in (x, y, s, P_bm))
            dA = torch.empty((K, B, self.nnz_aug), **f64)
            dq = torch.empty((K, B, self.n + 1), **f64)
            dP = torch.empty((K, B, self.nnz_p), **f64)
            adj = torch.empty((K, B), dtype=torch.int32, device=dev)
            rc = _lib.lib().ce_vjp_qp_many(self._h, B, K, A_c.data_ptr(), self.nnz_aug, P_c.data_ptr(), xc.data_ptr(), yc.data_ptr(), sc_.data_ptr(), dx.data_ptr(),
                                           None if dy is None else dy.data_ptr(), dA.data_ptr(), dq.data_ptr(), dP.data_ptr(), adj.data_ptr(), self._stream())
            _lib.check(rc, "ce_vjp_qp_many")
            return dA, dq, adj, dP
        if not (many or many_tri or many_psd):
            zero_dy = torch.zeros((B, self.m), **f64) if dy is None else None
            outs = [self.vjp(A_bm, x, y, s, dx[k], zero_dy if dy is None else dy[k], P_bm=P_bm, path=path, lsqr=lsqr, q_eval=q_eval) for k in range(K)]
            res = (torch.stack([o[0].t() for o in outs]).contiguous(), torch.stack([o[1].t() for o in outs]).contiguous(), torch.stack([o[2] for o in outs]))
            return res + ((torch.stack([o[3] for o in outs]),) if P_bm is not None else ())
        A_c = A_bm if (A_bm.stride(1) == 1 and (B == 1 or A_bm.stride(0) == self.nnz_aug)) else A_bm.contiguous()
        xc, yc, sc_ = (t.to(torch.float64).contiguous() for t in (x, y, s))
        qd, q_args = self._q_args(q_eval)
        rule = unpack_rule(lsqr, self.n, self.m)[:4]
        if rule[:3] != self._resolve_rule:
            _lib.check(_lib.lib().ce_set_adjoint_resolve(self._h, 1, float(rule[0]), float(rule[1]), 1e8, int(rule[2])), "ce_set_adjoint_resolve")
            self._resolve_rule = rule[:3]
        dA = torch.empty((K, B, self.nnz_aug), **f64)
        dq = torch.empty((K, B, self.n + 1), **f64)
        adj = torch.empty((K, B), dtype=torch.int32, device=dev)
        fn, name = ((_lib.lib().ce_vjp_psd_tri_many, "ce_vjp_psd_tri_many") if mixed else (_lib.lib().ce_vjp_psd_many, "ce_vjp_psd_many") if many_psd else
                    (_lib.lib().ce_vjp_tri_many, "ce_vjp_tri_many") if many_tri else (_lib.lib().ce_vjp_many, "ce_vjp_many"))
        rc = fn(self._h, B, K, A_c.data_ptr(), self.nnz_aug, *q_args, xc.data_ptr(), yc.data_ptr(), sc_.data_ptr(), dx.data_ptr(),
                None if dy is None else dy.data_ptr(), dA.data_ptr(), dq.data_ptr(), adj.data_ptr(), self._stream())
        _lib.check(rc, name)
        return dA, dq, adj

    @property
    def param_grad_variant(self) -> int:
        """>= 0: vjp_many_params / vjp_params serve this template (ce_param_grad_variant: exactly where ce_vjp_many_variant >= 0)"""
        return int(_lib.lib().ce_param_grad_variant(self._h))

    def _param_grad_prologue(self, maps, lsqr, q_eval, who, need_q: bool = True):
        if maps.n != self.n or maps.m != self.m or maps.nnz_aug != self.nnz_aug:
            raise ValueError(f"ConeEngine.{who}: the composed maps belong to another structure (n, m, nnz_aug) = ({maps.n}, {maps.m}, {maps.nnz_aug})")
        if getattr(maps, "nnz_p", 0) not in (0, self.nnz_p):
            raise ValueError(f"ConeEngine.{who}: the composed maps carry a P map of another structure (nnz_p = {maps.nnz_p}, the engine's is {self.nnz_p})")
        if not need_q:          # (the QP kind: no re-solve behind its launch)
            return maps.on(self.device)
        if q_eval is None:
            raise ValueError(f"ConeEngine.{who}: q_eval is required (the factor modes run in front of the armed LSQR re-solve)")
        rule = unpack_rule(lsqr, self.n, self.m)[:4]
        if rule[:3] != self._resolve_rule:
            _lib.check(_lib.lib().ce_set_adjoint_resolve(self._h, 1, float(rule[0]), float(rule[1]), 1e8, int(rule[2])), "ce_set_adjoint_resolve")
            self._resolve_rule = rule[:3]
        return maps.on(self.device)

    def vjp_many_params(self, A_bm, x, y, s, dx, dy, maps, lsqr: tuple | None = None, q_eval=None, out: torch.Tensor | None = None, P_bm=None,
                        qp_many: bool = False, tri_many: bool = False, psd_many: bool = False):
        """The parameter gradients of K cotangents at one solution, with no dA in memory: dx (K, B, n), dy (K, B, m) or None (zero), maps a
        param_grad.ComposedMaps of this template.  Returns g (K, B, maps.rows) -- written into `out` when given (contiguous, that shape) --, dq (K, B, n + 1) and
        adj (K, B).  g[k, b] is what the transposed parameter maps make of vjp_many's dA[k, b] and dq[k, b] (and dP[k, b]): to the bit on a parameter with one map
        entry, within the terms' rounding elsewhere.  One C call (last_vjp_many_path == "many_params", last_vjp_kernel names the entry): ce_vjp_many_params, or under
        the keywords of vjp_many the entry of that kind -- qp_many with P_bm: ce_vjp_qp_many_params (maps may carry a P map; q_eval and lsqr are not read: no
        re-solve); tri_many: ce_vjp_tri_many_params; psd_many: ce_vjp_psd_many_params, on a template with triples beside the blocks ce_vjp_psd_tri_many_params.
        The keyword SELECTS the entry: a template the entry does not serve raises _lib.EngineError with the library's reason and writes nothing."""
        dev = self.device
        f64 = dict(dtype=torch.float64, device=dev)
        K, B = int(dx.shape[0]), int(A_bm.shape[0])
        if qp_many and P_bm is None:
            raise ValueError("ConeEngine.vjp_many_params: qp_many needs P_bm")
        if sum(map(bool, (qp_many, tri_many, psd_many))) > 1 or (P_bm is not None and not qp_many):
            raise ValueError("ConeEngine.vjp_many_params: at most one of qp_many / tri_many / psd_many, and P_bm with qp_many alone")
        L = _lib.lib()
        name = ("ce_vjp_qp_many_params" if qp_many else "ce_vjp_tri_many_params" if tri_many else
                ("ce_vjp_psd_tri_many_params" if L.ce_vjp_psd_tri_many_variant(self._h) >= 0 else "ce_vjp_psd_many_params") if psd_many else "ce_vjp_many_params")
        ptr, code, kidx, val = self._param_grad_prologue(maps, lsqr, q_eval, "vjp_many_params", need_q=not qp_many)
        g = out if out is not None else torch.empty((K, B, maps.rows), **f64)
        if tuple(g.shape) != (K, B, maps.rows) or not g.is_contiguous() or g.dtype != torch.float64:
            raise ValueError(f"ConeEngine.vjp_many_params: out must be a contiguous float64 tensor of shape {(K, B, maps.rows)}")
        dq = torch.empty((K, B, self.n + 1), **f64)
        adj = torch.empty((K, B), dtype=torch.int32, device=dev)
        self.last_vjp_many_path, self.last_vjp_kernel = "many_params", name
        if B == 0 or K == 0:
            return g, dq, adj
        dx = dx.to(**f64).contiguous()
        dy = None if dy is None else dy.to(**f64).contiguous()
        A_c = A_bm if (A_bm.stride(1) == 1 and (B == 1 or A_bm.stride(0) == self.nnz_aug)) else A_bm.contiguous()
        xc, yc, sc_ = (t.detach().to(torch.float64).contiguous() for t in (x, y, s))
        map_args = (maps.rows, ptr.data_ptr(), code.data_ptr(), kidx.data_ptr(), val.data_ptr(), g.data_ptr(), dq.data_ptr(), adj.data_ptr(), self._stream())
        if qp_many:
            P_c = P_bm.detach().to(**f64).contiguous()
            rc = L.ce_vjp_qp_many_params(self._h, B, K, A_c.data_ptr(), self.nnz_aug, P_c.data_ptr(), xc.data_ptr(), yc.data_ptr(), sc_.data_ptr(), dx.data_ptr(),
                                         None if dy is None else dy.data_ptr(), *map_args)
        else:
            qd, q_args = self._q_args(q_eval)
            rc = getattr(L, name)(self._h, B, K, A_c.data_ptr(), self.nnz_aug, *q_args, xc.data_ptr(), yc.data_ptr(), sc_.data_ptr(), dx.data_ptr(),
                                  None if dy is None else dy.data_ptr(), *map_args)
        _lib.check(rc, name)
        return g, dq, adj

    def param_grad_records(self, K: int, B: int) -> torch.Tensor:
        """(K, B, m + 1 + n): the factor records (r_y, r_tau, r_x) the last vjp_many_params call of this size, of any kind, left in the engine (introspection for tests)"""
        out = torch.empty((K, B, self.m + 1 + self.n), dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().ce_param_grad_records(self._h, B, K, out.data_ptr(), self._stream()), "ce_param_grad_records")
        return out

    def vjp_params(self, A_bm, x, y, s, dx, dy, maps, lsqr: tuple | None = None, q_eval=None):
        """One cotangent: dx (B, n), dy (B, m).  Returns g (B, maps.rows), dq (n + 1, B), adj (B,) from ce_vjp_params -- the single-cotangent kernel in its factor
        mode and k_param_grad behind it (K = 1 of the many-mode is the slower kernel for one cotangent).  A value row shorter than m cannot carry the factors:
        that template takes vjp_many_params with K = 1."""
        dev = self.device
        B = int(A_bm.shape[0])
        if self.nnz_aug < self.m:
            g, dq, adj = self.vjp_many_params(A_bm, x, y, s, dx[None], None if dy is None else dy[None], maps, lsqr=lsqr, q_eval=q_eval)
            return g[0], dq[0].t(), adj[0]
        ptr, code, kidx, val = self._param_grad_prologue(maps, lsqr, q_eval, "vjp_params")
        g = torch.empty((B, maps.rows), dtype=torch.float64, device=dev)
        dq = torch.empty((self.n + 1, B), dtype=torch.float64, device=dev)
        adj = torch.empty((B,), dtype=torch.int32, device=dev)
        if B == 0:
            return g, dq, adj
        A_c = A_bm if (A_bm.stride(1) == 1 and (B == 1 or A_bm.stride(0) == self.nnz_aug)) else A_bm.contiguous()
        xc, yc, sc_, dxc, dyc = (t.to(torch.float64).contiguous() for t in (x, y, s, dx, dy))
        qd, q_args = self._q_args(q_eval)
        rc = _lib.lib().ce_vjp_params(self._h, B, A_c.data_ptr(), 1, self.nnz_aug, *q_args, xc.data_ptr(), yc.data_ptr(), sc_.data_ptr(), dxc.data_ptr(), dyc.data_ptr(),
                                      maps.rows, ptr.data_ptr(), code.data_ptr(), kidx.data_ptr(), val.data_ptr(), g.data_ptr(), dq.data_ptr(), B, 1, adj.data_ptr(),
                                      self._stream())
        _lib.check(rc, "ce_vjp_params")
        return g, dq, adj

    def _q_args(self, q_eval):
        """(tensor to keep alive, (pointer, stride0, stride1)) of an optional (n+1, B) objective as the C ABI takes it; None -> (None, (None, 0, 0))"""
        if q_eval is None:
            return None, (None, 0, 0)
        qd = q_eval.detach().to(dtype=torch.float64, device=self.device)
        return qd, (qd.data_ptr(), qd.stride(0), qd.stride(1))

    @contextmanager
    def _lsqr_variant(self, method: str):
        """the iterative adjoints run LSMR's recurrences inside the block ("lsmr"), LSQR's otherwise and after it (ce_set_lsqr_variant)"""
        _lib.check(_lib.lib().ce_set_lsqr_variant(self._h, 1 if method == "lsmr" else 0), "ce_set_lsqr_variant")
        try:
            yield
        finally:
            _lib.lib().ce_set_lsqr_variant(self._h, 0)

    def lsqr_one_kernel(self, fn, name, A_ptr, A_stride, B, x, y, s, dx, dy, batch_minor_out, atol, btol, iter_lim, q_eval, conlim):
        """The one-kernel LSQR adjoints, ce_vjp_lsqr (per-instance A) and ce_vjp_shared_a (one A): the same signature around the (A pointer, row stride) pair.
        Returns dA, dq, adj -- or None when the library says the template does not fit this kernel (rc -2 / -3: the caller falls through)."""
        dev = self.device
        f64 = dict(dtype=torch.float64, device=dev)
        dA_bm = torch.empty((B, self.nnz_aug), **f64); dq = torch.empty((self.n + 1, B), **f64)
        adj = torch.empty((B,), dtype=torch.int32, device=dev); its = torch.empty((B,), dtype=torch.int32, device=dev)
        xc, yc, sc_, dxc, dyc = (t.to(torch.float64).contiguous() for t in (x, y, s, dx, dy))
        qd, q_args = self._q_args(q_eval)
        rc = fn(self._h, B, A_ptr, A_stride, *q_args, xc.data_ptr(), yc.data_ptr(), sc_.data_ptr(), dxc.data_ptr(), dyc.data_ptr(),
                dA_bm.data_ptr(), dq.data_ptr(), B, 1, adj.data_ptr(), its.data_ptr(), float(atol), float(btol), float(conlim), int(iter_lim), self._stream())
        if rc in (-2, -3):
            return None
        _lib.check(rc, name)
        self.last_lsqr_iters = its
        return (dA_bm.t().contiguous() if batch_minor_out else dA_bm.t()), dq, adj

    def _vjp_lsqr(self, A_bm, x, y, s, dx, dy, batch_minor_out, atol, btol, iter_lim, q_eval, conlim=1e8):
        """ce_vjp_lsqr: one workgroup per instance runs Paige & Saunders' LSQR on diffcp's adjoint system M^T r = dz with THIS instance's A (include/cone_engine.h)"""
        B = A_bm.shape[0]
        A_c = A_bm if (A_bm.stride(1) == 1 and (B == 1 or A_bm.stride(0) >= self.nnz_aug)) else A_bm.contiguous()
        out = self.lsqr_one_kernel(_lib.lib().ce_vjp_lsqr, "ce_vjp_lsqr", A_c.data_ptr(), A_c.stride(0), B, x, y, s, dx, dy, batch_minor_out, atol, btol, iter_lim, q_eval, conlim)
        if out is None:          # CE_E_TOO_LARGE: mode="lsqr" cannot be honoured for this template
            _warn_once("lsqr_too_large", "MI355 solver: solver_args mode='lsqr' needs the LSQR vectors of one instance in LDS, which this template exceeds; "
                                         "falling back to the direct elimination (rank-deficient instances are flagged in info['adjoint'])")
        return out

    def jvp(self, A_bm, x, y, s, tA_bm, tq, path: str | None = None, lsqr: tuple | None = None, q_eval=None, conlim: float = 1e8, method: str = "lsqr",
            P_bm=None, tP_bm=None, psd_ns: bool = False):
        """Forward-mode derivative of the solution map (diffcp's `derivative`): tangents tA_bm (B, nnz_aug) of the value rows and tq (n+1, B) of q_eval, either may be
        None (zero).  Returns dx (B, n), dy (B, m), ds (B, m), status (B,) -- 1: LSQR hit its iteration limit -- and sets last_lsqr_iters.
        One kernel per call, ce_jvp_lsqr, or ce_jvp_shared_a when `path` is "const_a" (only the b entries of tA_bm are read there: a shared A has no tangent).
        path, lsqr (rule, adjoint_system) and q_eval as vjp(); the LSQR recurrences only.  NotImplementedError when the LSQR vectors of one instance exceed LDS.
        method="direct": ce_jvp on the per-instance path -- the search-free elimination, then LSQR under the same rule for the instances it flags rank deficient
        (status 4 | 8 and iterations > 0 there, status 0 and 0 iterations elsewhere).  Where the library has no elimination for the template, and on the const_a
        path, the LSQR call runs instead; last_jvp_kernel names the entry point that ran.
        P_bm (B, nnz_p): the quadratic objective of a qp_native engine, with its tangent tP_bm (or None: zero) -- method="direct" only: ce_jvp_qp, the same elimination
        with P inside and NO LSQR behind it (a flagged instance keeps the elimination's answer, status 4, 0 iterations); NotImplementedError under method="lsqr".
        psd_ns=True (with method="direct"): ce_jvp_psd in the place of ce_jvp -- the elimination with PSD blocks (psd_ns_plan()["psd_ns_variant"] >= 0), which
        ce_jvp refuses; the same fall to the LSQR call where the library has none for the template.  Without it a PSD template runs the LSQR call, as ever.
        On a template with PSD blocks AND triples (psd_tri_ns_variant >= 0) the flag calls ce_jvp_psd_tri, the elimination with both kinds."""
        if method not in ("lsqr", "direct"):
            raise ValueError(f"ConeEngine.jvp: method must be 'lsqr' or 'direct', got {method!r}")
        B = A_bm.shape[0]
        dev = self.device
        f64 = dict(dtype=torch.float64, device=dev)
        if B == 0:
            return torch.empty((0, self.n), **f64), torch.empty((0, self.m), **f64), torch.empty((0, self.m), **f64), torch.empty((0,), dtype=torch.int32, device=dev)
        if path is None:
            path = self.last_path
        if P_bm is not None:
            if method != "direct":
                raise NotImplementedError("ConeEngine.jvp: a quadratic objective inside the kernels has no LSQR forward derivative; use method='direct' "
                                          "(or the epigraph form, CE_QP_EPIGRAPH=1)")
            return self._jvp_qp(A_bm, P_bm, x, y, s, tA_bm, tq, tP_bm)
        atol, btol, lim, system, _ = unpack_rule(lsqr, self.n, self.m)
        if q_eval is None and system != "reduced":
            q_eval = self._recent_q(A_bm)
        if system == "reduced":
            q_eval = None
        shared = path == "const_a"
        fn, name = (_lib.lib().ce_jvp_shared_a, "ce_jvp_shared_a") if shared else (_lib.lib().ce_jvp_lsqr, "ce_jvp_lsqr")
        A_c = A_bm if (A_bm.stride(1) == 1 and (B == 1 or A_bm.stride(0) >= self.nnz_aug)) else A_bm.contiguous()
        point, tangents, outs, keep = self._jvp_buffers(B, x, y, s, tA_bm, tq)
        qd, q_args = self._q_args(q_eval)
        dx, dy, ds, st, its = outs
        def call(fn, A_t):
            return fn(self._h, B, A_t.data_ptr(), A_t.stride(0), *q_args, *point, *tangents, *(t.data_ptr() for t in outs),
                      float(atol), float(btol), float(conlim), int(lim), self._stream())
        rc = -2
        if method == "direct" and not shared:
            direct, dname = (((_lib.lib().ce_jvp_psd_tri, "ce_jvp_psd_tri") if self.psd_tri_ns_variant >= 0 else (_lib.lib().ce_jvp_psd, "ce_jvp_psd")) if psd_ns
                             else (_lib.lib().ce_jvp, "ce_jvp"))
            rc = call(direct, A_c if A_c.stride(0) == self.nnz_aug else A_c.contiguous())
            if rc != -2:          # (CE_E_UNSUPPORTED: no elimination for this template -- the LSQR call below serves it)
                name = dname
        if rc == -2:
            rc = call(fn, A_c)
        if rc in (-2, -3):
            raise NotImplementedError(_lib.lib().ce_last_error().decode())
        _lib.check(rc, name)
        self.last_jvp_kernel = name
        self.last_lsqr_iters = its
        return dx, dy, ds, st

    def jvp_many(self, A_bm, x, y, s, tA, tq, path: str | None = None, lsqr: tuple | None = None, q_eval=None, conlim: float = 1e8, method: str = "direct",
                 P_bm=None, tP=None, force_loop: bool = False, tri_many: bool = False, psd_many: bool = False):
        """K tangents at one solution.  tA (K, B, nnz_aug), tq (K, B, n+1), tP (K, B, nnz_p) -- or (K, .) for a tangent every instance shares (batch stride 0: a
        parameter-space basis vector pushed through the parameter maps); at most two of the three may be None (zero).  Returns dx (K, B, n), dy (K, B, m),
        ds (K, B, m), status (K, B) and sets last_lsqr_iters (K, B): for every k what jvp(method=method) returns for the k-th tangent.
        One C call (each instance factored once, last_jvp_many_path == "many") under the rule that sends jvp(method="direct") to ce_jvp / ce_jvp_qp -- ce_jvp_qp_many with
        P_bm, ce_jvp_many on every path but "const_a" -- when the kind's *_many_variant >= 0.  Every other case (method="lsqr", the shared-A path, PSD cones or
        triples, templates without the mode, force_loop) is K calls of jvp, stacked ("loop"): the method is total wherever jvp is, and the loop is the comparator.
        tri_many (opt-in, default False): on a template with exponential / power triples (ce_jvp_tri_many_variant >= 0), method "direct", no P_bm, any path but
        "const_a", one ce_jvp_tri_many call instead of the K ce_jvp calls (last_jvp_many_path == "many", last_jvp_kernel == "ce_jvp_tri_many"): each triple is
        diagonalised and rotated and each instance factored once for all K tangents, and one LSQR launch re-solves the flagged instances for every k.  Flags and
        the re-solve's answers are those of the loop.  In every other case the flag changes nothing.
        psd_many (opt-in, default False): on a template with PSD blocks (ce_jvp_psd_many_variant >= 0), under tri_many's conditions, one ce_jvp_psd_many call
        (last_jvp_kernel == "ce_jvp_psd_many") instead of the K calls of the loop, which are ce_jvp_lsqr calls on such a template: each block is decomposed, its rows
        rotated and each instance factored once for all K tangents.  With force_loop the flag selects the loop's kernel instead: K ce_jvp_psd calls, the elimination
        this mode repeats K times less -- its comparator.  In every other case the flag changes nothing.  On a template with PSD blocks AND triples
        (ce_jvp_psd_tri_many_variant >= 0) the one call is ce_jvp_psd_tri_many and the loop under force_loop is K ce_jvp_psd_tri calls."""
        if method not in ("lsqr", "direct"):
            raise ValueError(f"ConeEngine.jvp_many: method must be 'lsqr' or 'direct', got {method!r}")
        given = [t for t in (tA, tq, tP) if t is not None]
        if not given:
            raise ValueError("ConeEngine.jvp_many: at least one of tA, tq, tP must be given (K is their leading dimension)")
        K, B = int(given[0].shape[0]), int(A_bm.shape[0])
        if any(int(t.shape[0]) != K for t in given):
            raise ValueError("ConeEngine.jvp_many: the tangents disagree on K")
        if tP is not None and P_bm is None:
            raise ValueError("ConeEngine.jvp_many: tP needs P_bm")
        dev = self.device
        f64 = dict(dtype=torch.float64, device=dev)
        if path is None:
            path = self.last_path
        L = _lib.lib()
        many = not force_loop and method == "direct" and (L.ce_jvp_qp_many_variant(self._h) >= 0 if P_bm is not None else (path != "const_a" and L.ce_jvp_many_variant(self._h) >= 0))
        many_tri = (not force_loop and tri_many and not many and method == "direct" and P_bm is None and path != "const_a"
                    and L.ce_jvp_tri_many_variant(self._h) >= 0)
        psd_ok = (psd_many and not many and not many_tri and method == "direct" and P_bm is None and path != "const_a"
                  and (L.ce_jvp_psd_many_variant(self._h) >= 0 or L.ce_jvp_psd_tri_many_variant(self._h) >= 0))
        many_psd = psd_ok and not force_loop
        mixed = many_psd and L.ce_jvp_psd_tri_many_variant(self._h) >= 0          # (PSD blocks and triples: the mixed entry, the same arguments)
        many = many or many_tri or many_psd
        self.last_jvp_many_path = "many" if many else "loop"
        i32 = dict(dtype=torch.int32, device=dev)
        if B == 0 or K == 0:
            self.last_lsqr_iters = torch.empty((K, B), **i32)
            return torch.empty((K, B, self.n), **f64), torch.empty((K, B, self.m), **f64), torch.empty((K, B, self.m), **f64), torch.empty((K, B), **i32)
        tA, tq, tP = (None if t is None else t.detach().to(**f64).contiguous() for t in (tA, tq, tP))
        if not many:
            def of(t, k):          # tangent k as jvp takes it: one row per instance
                return None if t is None else (t[k] if t.dim() == 3 else t[k].unsqueeze(0).expand(B, -1))
            outs, its = [], []
            for k in range(K):
                tqk = of(tq, k)
                outs.append(self.jvp(A_bm, x, y, s, of(tA, k), None if tqk is None else tqk.t(), path=path, lsqr=lsqr, q_eval=q_eval, conlim=conlim, method=method,
                                     P_bm=P_bm, tP_bm=of(tP, k), psd_ns=psd_ok))
                its.append(self.last_lsqr_iters)
            self.last_lsqr_iters = torch.stack(its)
            return tuple(torch.stack([o[i] for o in outs]) for i in range(4))
        def strides(t, row):          # (pointer, tangent stride, batch stride) of a (K, B, row) or (K, row) tangent
            return (None, 0, 0) if t is None else (t.data_ptr(), t.stride(0), row if t.dim() == 3 else 0)
        A_c = A_bm.detach().to(**f64)
        A_c = A_c if (A_c.stride(1) == 1 and (B == 1 or A_c.stride(0) == self.nnz_aug)) else A_c.contiguous()
        xc, yc, sc_ = (t.detach().to(**f64).contiguous() for t in (x, y, s))
        dx, dy, ds = torch.empty((K, B, self.n), **f64), torch.empty((K, B, self.m), **f64), torch.empty((K, B, self.m), **f64)
        st, its = torch.empty((K, B), **i32), torch.empty((K, B), **i32)
        outp = (dx.data_ptr(), dy.data_ptr(), ds.data_ptr(), st.data_ptr(), its.data_ptr())
        if P_bm is not None:
            P_c = P_bm.detach().to(**f64).contiguous()
            rc, name = L.ce_jvp_qp_many(self._h, B, K, A_c.data_ptr(), self.nnz_aug, P_c.data_ptr(), xc.data_ptr(), yc.data_ptr(), sc_.data_ptr(),
                                        *strides(tA, self.nnz_aug), *strides(tq, self.n + 1), *strides(tP, self.nnz_p), *outp, self._stream()), "ce_jvp_qp_many"
        else:
            atol, btol, lim, system, _ = unpack_rule(lsqr, self.n, self.m)
            if q_eval is None and system != "reduced":
                q_eval = self._recent_q(A_bm)
            if system == "reduced":
                q_eval = None
            qd, q_args = self._q_args(q_eval)
            fn, name = ((L.ce_jvp_psd_tri_many, "ce_jvp_psd_tri_many") if mixed else (L.ce_jvp_psd_many, "ce_jvp_psd_many") if many_psd else
                        (L.ce_jvp_tri_many, "ce_jvp_tri_many") if many_tri else (L.ce_jvp_many, "ce_jvp_many"))
            rc = fn(self._h, B, K, A_c.data_ptr(), self.nnz_aug, *q_args, xc.data_ptr(), yc.data_ptr(), sc_.data_ptr(),
                    *strides(tA, self.nnz_aug), *strides(tq, self.n + 1), *outp, float(atol), float(btol), float(conlim), int(lim), self._stream())
        _lib.check(rc, name)
        self.last_jvp_kernel = name
        self.last_lsqr_iters = its
        return dx, dy, ds, st

    def _jvp_buffers(self, B, x, y, s, tA_bm, tq):
        """What every forward-derivative entry point takes: the pointers of the point (x, y, s), of the tangents (tA, its row stride, tq and its strides), the output
        tensors dx, dy, ds, status, iterations, and the converted inputs, which the caller keeps alive until the call returns"""
        f64 = dict(dtype=torch.float64, device=self.device)
        xc, yc, sc_ = (t.detach().to(**f64).contiguous() for t in (x, y, s))
        tA_c = tA_bm.detach().to(**f64).contiguous() if tA_bm is not None else None
        tqd, tq_args = self._q_args(tq)
        outs = (torch.empty((B, self.n), **f64), torch.empty((B, self.m), **f64), torch.empty((B, self.m), **f64),
                torch.empty((B,), dtype=torch.int32, device=self.device), torch.empty((B,), dtype=torch.int32, device=self.device))
        point = (xc.data_ptr(), yc.data_ptr(), sc_.data_ptr())
        tangents = (tA_c.data_ptr() if tA_c is not None else None, self.nnz_aug, *tq_args)
        return point, tangents, outs, (xc, yc, sc_, tA_c, tqd)

    def _jvp_qp(self, A_bm, P_bm, x, y, s, tA_bm, tq, tP_bm):
        """ce_jvp_qp (include/cone_engine.h): one launch of the search-free elimination with P inside"""
        B = A_bm.shape[0]
        f64 = dict(dtype=torch.float64, device=self.device)
        A_c, P_c = (t.detach().to(**f64).contiguous() for t in (A_bm, P_bm))
        tP_c = tP_bm.detach().to(**f64).contiguous() if tP_bm is not None else None
        point, tangents, outs, keep = self._jvp_buffers(B, x, y, s, tA_bm, tq)
        dx, dy, ds, st, its = outs
        rc = _lib.lib().ce_jvp_qp(self._h, B, A_c.data_ptr(), self.nnz_aug, P_c.data_ptr(), *point, *tangents, tP_c.data_ptr() if tP_c is not None else None,
                                  *(t.data_ptr() for t in outs), self._stream())
        if rc == -2:
            raise NotImplementedError(_lib.lib().ce_last_error().decode())
        _lib.check(rc, "ce_jvp_qp")
        self.last_jvp_kernel = "ce_jvp_qp"
        self.last_lsqr_iters = its
        return dx, dy, ds, st

    def refine(self, A_bm, q_eval, x, y, s, steps: int, status=None, P_bm=None, psd_ns: bool = False):
        """`steps` safeguarded Newton steps on the KKT residual of (x, y, s) (include/cone_engine.h ce_refine): A_bm (B, nnz_aug), q_eval (n+1, B), x (B, n), y, s
        (B, m); status (B,) int32 or None: instances with a negative forward status are skipped.  Returns x, y, s, info -- contiguous fp64 tensors on this
        engine's device are refined IN PLACE and handed back, others are copied first.  info: "status" (bits 1 a step kept, 2 a step rejected, 4 flagged by the
        elimination, 16 skipped), "steps" (kept per instance), "resid_before" / "resid_after" (rho of the point that came in and of the one returned), "path"
        "ns" -- or "none", with the other entries None and the point untouched, where the library has no elimination for the template.  No host synchronisation.
        P_bm (B, nnz_p): the quadratic objective of a qp_native engine (ce_refine_qp: F_x = P x + A^T y^ + c).
        psd_ns=True: ce_refine_psd in the place of ce_refine -- the elimination with PSD blocks, which ce_refine refuses (path "none" without the flag)."""
        B = A_bm.shape[0]
        dev = self.device
        f64 = dict(dtype=torch.float64, device=dev)
        none = {"status": None, "steps": None, "resid_before": None, "resid_after": None, "path": "none"}
        if B == 0 or int(steps) <= 0:
            return x, y, s, none
        x, y, s = (t.detach().to(**f64).contiguous() for t in (x, y, s))
        A_c = A_bm if (A_bm.is_contiguous() and A_bm.dtype == torch.float64) else A_bm.to(torch.float64).contiguous()
        qd, q_args = self._q_args(q_eval)
        st_c = status.to(device=dev, dtype=torch.int32).contiguous() if status is not None else None
        rst = torch.empty((B,), dtype=torch.int32, device=dev); taken = torch.empty((B,), dtype=torch.int32, device=dev)
        resid = torch.empty((B, 2), **f64)
        tail = (x.data_ptr(), y.data_ptr(), s.data_ptr(), st_c.data_ptr() if st_c is not None else None, int(steps), rst.data_ptr(), taken.data_ptr(), resid.data_ptr(), self._stream())
        if P_bm is not None:
            P_c = P_bm.detach().to(**f64).contiguous()
            rc, name = _lib.lib().ce_refine_qp(self._h, B, A_c.data_ptr(), self.nnz_aug, *q_args, P_c.data_ptr(), *tail), "ce_refine_qp"
        elif psd_ns and self.psd_tri_ns_variant >= 0:          # (PSD blocks and triples: the mixed entry, the same arguments)
            rc, name = _lib.lib().ce_refine_psd_tri(self._h, B, A_c.data_ptr(), self.nnz_aug, *q_args, *tail), "ce_refine_psd_tri"
        elif psd_ns:
            rc, name = _lib.lib().ce_refine_psd(self._h, B, A_c.data_ptr(), self.nnz_aug, *q_args, *tail), "ce_refine_psd"
        else:
            rc, name = _lib.lib().ce_refine(self._h, B, A_c.data_ptr(), self.nnz_aug, *q_args, *tail), "ce_refine"
        if rc == -2:
            return x, y, s, none
        _lib.check(rc, name)
        return x, y, s, {"status": rst, "steps": taken, "resid_before": resid[:, 0], "resid_after": resid[:, 1], "path": "ns"}

    def check_solved(self, A_eval, q_eval, x, y, s, eps_abs: float, eps_rel: float, eligible=None, eligible_mask: int = 1, P_bm=None, p_structure=None,
                     status=None, iters=None, resid=None):
        """The forward kernels' termination test at the point (x (B, n), y, s (B, m)) (include/cone_engine.h ce_check_solved).  A_eval (nnz_aug, B), q_eval
        (n+1, B) fp64 on this engine's device in ANY strides (nothing is copied); P_bm (B, nnz_p) contiguous with p_structure = (p_rows, p_cols) int32 device
        tensors; eligible (B,) int32 or None: an instance with eligible & eligible_mask == 0 is unsolved whatever its residual.  Returns solved (B,) uint8,
        status, iters (B,) int32, resid (B, 3), n_unsolved (1,) int32 ON THE DEVICE: a solved instance gets status 1, iters 0 and its resid row, every other
        entry of status / iters / resid keeps what the given tensor held (new tensors: zeros).  Enqueues only."""
        B = x.shape[0]
        dev = self.device
        i32 = dict(dtype=torch.int32, device=dev)
        solved = torch.empty((B,), dtype=torch.uint8, device=dev)
        status = torch.zeros((B,), **i32) if status is None else status
        iters = torch.zeros((B,), **i32) if iters is None else iters
        resid = torch.zeros((B, 3), dtype=torch.float64, device=dev) if resid is None else resid
        if B == 0:
            return solved, status, iters, resid, torch.zeros((1,), **i32)
        n_uns = torch.empty((1,), **i32)
        for name, t, dt in (("x", x, torch.float64), ("y", y, torch.float64), ("s", s, torch.float64), ("status", status, torch.int32), ("iters", iters, torch.int32),
                            ("resid", resid, torch.float64)) + ((("eligible", eligible, torch.int32),) if eligible is not None else ()):
            if t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"ConeEngine.check_solved: {name} must be a contiguous {dt} tensor on {dev}")
        if tuple(x.shape) != (B, self.n) or tuple(y.shape) != (B, self.m) or tuple(s.shape) != (B, self.m) or tuple(A_eval.shape) != (self.nnz_aug, B) or \
                tuple(q_eval.shape) != (self.n + 1, B) or status.numel() != B or iters.numel() != B or tuple(resid.shape) != (B, 3) or (eligible is not None and eligible.numel() != B):
            raise ValueError("ConeEngine.check_solved: shapes do not match the template and the batch size")
        pr, pc, nnz_p = self._p_args(p_structure if P_bm is not None else None)
        rc = _lib.lib().ce_check_solved(self._h, B, A_eval.data_ptr(), A_eval.stride(0), A_eval.stride(1), q_eval.data_ptr(), q_eval.stride(0), q_eval.stride(1),
                                        P_bm.data_ptr() if nnz_p else None, pr, pc, nnz_p, x.data_ptr(), y.data_ptr(), s.data_ptr(),
                                        eligible.data_ptr() if eligible is not None else None, int(eligible_mask), float(eps_abs), float(eps_rel),
                                        solved.data_ptr(), status.data_ptr(), iters.data_ptr(), resid.data_ptr(), n_uns.data_ptr(), self._stream())
        _lib.check(rc, "ce_check_solved")
        return solved, status, iters, resid, n_uns

    # ---- the optimal value and its envelope-theorem derivatives (include/cone_engine.h ce_value ...): streaming passes, no system solved
    @staticmethod
    def _p_args(p_structure):
        """(p_rows, p_cols) int32 device tensors or None -> (rows pointer, cols pointer, nnz_p) as the C ABI takes the P structure"""
        if p_structure is None or p_structure[0].numel() == 0:
            return None, None, 0
        return p_structure[0].data_ptr(), p_structure[1].data_ptr(), int(p_structure[0].numel())

    def value(self, A_eval, q_eval, x, y, P_bm=None, p_structure=None):
        """pobj, dobj (B,) of the point (x (B, n), y (B, m)): c^T x + d + 1/2 x^T P x and -b^T y - 1/2 x^T P x + d.  A_eval (nnz_aug, B), q_eval (n+1, B) fp64 on
        this engine's device in ANY strides (nothing is copied); P_bm (B, nnz_p) contiguous with p_structure = (p_rows, p_cols) int32 device tensors."""
        B = x.shape[0]
        f64 = dict(dtype=torch.float64, device=self.device)
        pobj, dobj = torch.empty((B,), **f64), torch.empty((B,), **f64)
        if B == 0:
            return pobj, dobj
        pr, pc, nnz_p = self._p_args(p_structure if P_bm is not None else None)
        rc = _lib.lib().ce_value(self._h, B, A_eval.data_ptr(), A_eval.stride(0), A_eval.stride(1), q_eval.data_ptr(), q_eval.stride(0), q_eval.stride(1),
                                 P_bm.data_ptr() if nnz_p else None, pr, pc, nnz_p, x.data_ptr(), y.data_ptr(), pobj.data_ptr(), dobj.data_ptr(), self._stream())
        _lib.check(rc, "ce_value")
        return pobj, dobj

    def value_jvp(self, x, y, tA_bm=None, tq=None, tP_bm=None, p_structure=None):
        """The tangent (B,) of the optimal value for tangents tA_bm (B, nnz_aug) batch-major rows, tq (n+1, B) in any strides, tP_bm (B, nnz_p); None = zero."""
        B = x.shape[0]
        tval = torch.empty((B,), dtype=torch.float64, device=self.device)
        if B == 0:
            return tval
        pr, pc, nnz_p = self._p_args(p_structure if tP_bm is not None else None)
        tqd, tq_args = self._q_args(tq)
        rc = _lib.lib().ce_value_jvp(self._h, B, tA_bm.data_ptr() if tA_bm is not None else None, tA_bm.stride(0) if tA_bm is not None else 0, *tq_args,
                                     tP_bm.data_ptr() if nnz_p else None, pr, pc, nnz_p, x.data_ptr(), y.data_ptr(), tval.data_ptr(), self._stream())
        _lib.check(rc, "ce_value_jvp")
        return tval

    def value_vjp(self, x, y, g, skip=None, want=(True, True, True), batch_minor_A: bool = False, batch_minor_q: bool = True, p_structure=None):
        """dA (nnz_aug, B), dq (n+1, B), dP (B, nnz_p) of the optimal value for the cotangent g (B,); want = (dA, dq, dP): the others come back None.
        batch_minor_A / batch_minor_q: the tensor is (., B) contiguous; otherwise the transposed view of a batch-major buffer (the engine-native layout).
        skip (B,) bool / uint8 or None: those instances get exact zeros."""
        B = x.shape[0]
        f64 = dict(dtype=torch.float64, device=self.device)
        pr, pc, nnz_p = self._p_args(p_structure if want[2] else None)
        dA = dq = dP = None
        sA = sq = (0, 0)
        if want[0]:
            dA, sA = (torch.empty((self.nnz_aug, B), **f64), (B, 1)) if batch_minor_A else (torch.empty((B, self.nnz_aug), **f64).t(), (1, self.nnz_aug))
        if want[1]:
            dq, sq = (torch.empty((self.n + 1, B), **f64), (B, 1)) if batch_minor_q else (torch.empty((B, self.n + 1), **f64).t(), (1, self.n + 1))
        if nnz_p:
            dP = torch.empty((B, nnz_p), **f64)
        if B == 0 or (dA is None and dq is None and dP is None):
            return dA, dq, dP
        sk = skip.view(torch.uint8) if (skip is not None and skip.dtype == torch.bool) else skip
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = _lib.lib().ce_value_vjp(self._h, B, x.data_ptr(), y.data_ptr(), g.data_ptr(), ptr(sk), ptr(dA), *sA, ptr(dq), *sq, ptr(dP), pr, pc, nnz_p, self._stream())
        _lib.check(rc, "ce_value_vjp")
        return dA, dq, dP

    # introspection (bench / tests)
    def set_profiling(self, on):
        """False / True, or a sum of 2 (forward), 4 (adjoint), 8 (layout passes): which launches are bracketed by HIP events (include/cone_engine.h)"""
        _lib.lib().ce_set_profiling(self._h, int(on))

    def reset_profile(self):
        _lib.lib().ce_reset_profile(self._h)

    def profile(self, which: int):
        ms, nl = C.c_double(), C.c_int()
        _lib.check(_lib.lib().ce_get_profile(self._h, which, C.byref(ms), C.byref(nl)), "ce_get_profile")
        return ms.value, nl.value

    def launch_info(self):
        """LDS footprints and modes of the launch plan, read once at construction (a copy: callers may keep or change it)"""
        return dict(self._launch_info)

    PLAN_FIELDS = ("fwd_mode", "f2_variant", "rt_variant", "wl", "aa_ok", "gen_blocked_f", "qp_native",
                   "bwd_mode", "brt_variant", "two_tile", "ns_variant", "gen_blocked_b", "sp_r", "sp_RP", "last_fast",
                   "last_sa_fwd", "last_sa_lsqr", "tri_ns_variant")

    def plan(self):
        """The whole launch plan (include/cone_engine.h ce_get_plan) as a dict keyed by PLAN_FIELDS.  Read from the library on every call, unlike
        launch_info(): the last_* entries change from call to call -- last_fast is the first tile of the most recent two-tile adjoint call, last_sa_fwd /
        last_sa_lsqr the rows of csrc/ce_variants.h the most recent shared-A forward / LSQR launch ran (tests/test_gpu_plan_edges.py reads them between calls).  Nothing on the solve / vjp path calls this."""
        L = _lib.lib()
        cnt = L.ce_get_plan(self._h, None, 0)
        _lib.check(min(cnt, 0), "ce_get_plan")
        buf = (C.c_int * cnt)()
        L.ce_get_plan(self._h, buf, cnt)
        return dict(zip(self.PLAN_FIELDS, list(buf)))

    def psd_tri_ns_plan(self):
        """The plan of the opt-in search-free elimination with PSD blocks AND exponential / power triples (ce_jvp_psd_tri, ce_refine_psd_tri, ce_vjp_psd_tri_many,
        ce_jvp_psd_tri_many), which ce_get_plan and PLAN_FIELDS do not carry: "psd_tri_ns_variant" (row of CE_NS_VARIANTS, -1: the template is not served) and
        "psd_tri_ns_lds" (its LDS footprint in bytes, 0: none)."""
        L = _lib.lib()
        return {"psd_tri_ns_variant": int(L.ce_psd_tri_ns_variant(self._h)), "psd_tri_ns_lds": int(L.ce_psd_tri_ns_lds(self._h))}

    def psd_ns_plan(self):
        """The plan of the opt-in search-free elimination with PSD blocks (ce_jvp_psd / ce_refine_psd), which ce_get_plan and PLAN_FIELDS do not carry:
        "psd_ns_variant" (row of CE_NS_VARIANTS, -1: the template is not served) and "psd_ns_lds" (its LDS footprint in bytes, 0: none)."""
        L = _lib.lib()
        return {"psd_ns_variant": int(L.ce_psd_ns_variant(self._h)), "psd_ns_lds": int(L.ce_psd_ns_lds(self._h))}

"""optimal_value: the optimal value p* = c^T x* + d (+ 1/2 x*^T P x*) of a solved layer as a differentiable output, with envelope-theorem gradients.

By the envelope theorem the TOTAL derivative of p* with respect to the problem data is the PARTIAL derivative of the Lagrangian at (x*, y*): in solver form
(A x + s = b)  dp*/dA = y x^T, dp*/db = -y, dp*/dc = x, dp*/dd = 1, dp*/dP = 1/2 x x^T.  No linear system is solved, so nothing can be rank deficient, every
cone kind and every path of the engine is served (plain cones, PSD, exponential / power, P inside the kernels or as an epigraph, shared A), and the cost is
one streaming pass (include/cone_engine.h ce_value, ce_value_jvp, ce_value_vjp).

The function sits BEHIND `_CvxpyLayer.apply`, whose four outputs stay as they are: it takes the ORIGINAL P_eval / q_eval / A_eval and the primal, dual that
call returned.  primal and dual enter DETACHED: the envelope gradient is the total derivative already, and letting it also flow through x*, y* would count
the (vanishing) solution path a second time and launch the adjoint.
"""
from __future__ import annotations

import numpy as np
import torch


def _p_structure(ctx, device):
    """(p_rows, p_cols) of the context's P structure as int32 tensors on `device` (cached on the context), or None without a quadratic objective"""
    if ctx.quad is None:
        return None
    cache = ctx.__dict__.setdefault("_value_pst", {})
    key = str(device)
    if key not in cache:
        cache[key] = (torch.from_numpy(np.asarray(ctx.quad.p_rows, dtype=np.int32)).to(device), torch.from_numpy(np.asarray(ctx.quad.p_cols, dtype=np.int32)).to(device))
    return cache[key]


def _batch_major(t: torch.Tensor) -> torch.Tensor:
    """(K, B) in any layout -> (B, K) contiguous; zero-copy for a batch-minor view of batch-major storage (the frontend's A_bm.t())"""
    return t.t().contiguous()


class _OptimalValue(torch.autograd.Function):

    @staticmethod
    def forward(P_eval, q_eval, A_eval, primal, dual, cl_ctx, failed, info):
        ctx = cl_ctx.solver_ctx if hasattr(cl_ctx, "solver_ctx") else cl_ctx
        if not torch.cuda.is_available():
            raise RuntimeError("MI355 solver needs a ROCm GPU; there is no CPU fallback (use solver='DIFFCP' on CPU)")
        unbatched = A_eval.dim() == 1
        if unbatched:
            A_eval, q_eval = A_eval.unsqueeze(1), q_eval.unsqueeze(1)
            P_eval = P_eval.unsqueeze(1) if P_eval is not None else None
        in_device = A_eval.device
        dev = in_device if in_device.type == "cuda" else ctx.default_device
        eng = ctx.engine(dev)
        f64 = dict(device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            A_dev, q_dev = A_eval.detach().to(**f64), q_eval.detach().to(**f64)
            x = primal.detach().to(**f64).reshape(-1, eng.n).contiguous()
            y = dual.detach().to(**f64).reshape(-1, eng.m).contiguous()
            if x.shape[0] != A_dev.shape[1] or y.shape[0] != A_dev.shape[1]:
                raise ValueError(f"optimal_value: primal / dual hold {x.shape[0]} / {y.shape[0]} instances, A_eval {A_dev.shape[1]}")
            pst = _p_structure(ctx, dev) if P_eval is not None else None
            P_bm = _batch_major(P_eval.detach().to(**f64)) if pst is not None else None
            pobj, dobj = eng.value(A_dev, q_dev, x, y, P_bm=P_bm, p_structure=pst)
            fail = failed.to(device=dev, dtype=torch.bool).reshape(-1) if failed is not None else None
            val = pobj if fail is None else torch.where(fail, float("nan"), pobj)
        if isinstance(info, dict):
            info["objective"] = {"primal": pobj.reshape(()) if unbatched else pobj, "dual": dobj.reshape(()) if unbatched else dobj}
        # batch-minor views of batch-major storage get their gradient in the same storage order (no layout pass, no strided accumulation)
        layout = (A_dev.shape[1] > 1 and A_dev.stride(0) != 1, q_dev.shape[1] == 1 or q_dev.stride(0) != 1)
        saved = (eng, x, y, fail, pst, unbatched, in_device, layout)
        out = val.to(in_device)
        return (out.reshape(()) if unbatched else out), saved

    @staticmethod
    def setup_context(ctx, inputs, outputs):
        ctx.saved = outputs[1]
        ctx.set_materialize_grads(False)

    @staticmethod
    def jvp(ctx, tP, tq, tA, *_):
        eng, x, y, fail, pst, unbatched, in_device, _layout = ctx.saved
        if tq is None and tA is None and (tP is None or pst is None):
            return None, None
        f64 = dict(device=eng.device, dtype=torch.float64)
        with torch.cuda.device(eng.device):
            def bm(t):
                return _batch_major((t.unsqueeze(1) if unbatched else t).detach().to(**f64)) if t is not None else None
            tq_dev = (tq.unsqueeze(1) if unbatched else tq).detach().to(**f64) if tq is not None else None
            tval = eng.value_jvp(x, y, tA_bm=bm(tA), tq=tq_dev, tP_bm=bm(tP) if pst is not None else None, p_structure=pst)
            if fail is not None:
                tval = torch.where(fail, float("nan"), tval)
        tval = tval.to(in_device)
        return (tval.reshape(()) if unbatched else tval), None

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _saved):
        eng, x, y, fail, pst, unbatched, in_device, (bmin_A, bmin_q) = ctx.saved
        if g is None:
            return (None,) * 8
        want = (ctx.needs_input_grad[2], ctx.needs_input_grad[1], ctx.needs_input_grad[0] and pst is not None)
        with torch.cuda.device(eng.device):
            g_dev = g.detach().to(device=eng.device, dtype=torch.float64).reshape(-1).contiguous()
            dA, dq, dP = eng.value_vjp(x, y, g_dev, skip=fail, want=want, batch_minor_A=bmin_A, batch_minor_q=bmin_q, p_structure=pst)
        dA = dA.to(in_device) if dA is not None else None
        dq = dq.to(in_device) if dq is not None else None
        dP = dP.t().to(in_device) if dP is not None else None
        if unbatched:
            dA, dq, dP = (t.squeeze(1) if t is not None else None for t in (dA, dq, dP))
        return dP, dq, dA, None, None, None, None, None


def optimal_value(P_eval, q_eval, A_eval, primal, dual, cl_ctx, failed=None, info=None):
    """The optimal value of the solved instances, (B,) float64 -- or () for unbatched inputs --, differentiable with respect to P_eval, q_eval, A_eval
    (reverse mode: ce_value_vjp; torch.autograd.forward_ad: ce_value_jvp).

    P_eval / q_eval / A_eval: what `_CvxpyLayer.apply` was called with (P_eval None for a linear objective); batch-minor views of batch-major storage
    (A_bm.t()) are read and differentiated without a copy.  primal, dual: what that call returned; they are detached here.
    failed (B,) bool or None: instances the solver masked (solver_args raise_on_error=False, info["status"] < 0) return NaN and contribute exact zeros to the
    gradients.  info: a dict that receives info["objective"] = {"primal": c^T x + d + 1/2 x^T P x, "dual": -b^T y - 1/2 x^T P x + d} (detached; equal at a solution)."""
    val, _ = _OptimalValue.apply(P_eval, q_eval, A_eval, primal.detach(), dual.detach(), cl_ctx, failed, info)
    return val

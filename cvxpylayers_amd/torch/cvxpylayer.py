"""PyTorch frontend for the MI355 engine, mirroring cvxpylayers.torch.CvxpyLayer
(reference: src/cvxpylayers/torch/cvxpylayer.py:285-490) for the one solver key this repository provides.

What is the same as the reference (argument meaning, shapes, errors):
  * CvxpyLayer(...).forward(*params, solver_args=None): one tensor per parameter, each with the parameter's shape or
    with one leading batch axis; batched and unbatched parameters may be mixed (unbatched ones are broadcast); all batched
    parameters must share the batch size; wrong counts / shapes raise ValueError with the reference's messages
    (utils/parse_args.py:94-143).
  * parameters are flattened in Fortran order, stacked in the canonical column order, followed by a constant 1
    (torch/cvxpylayer.py:84-141), and pushed through the affine parameter maps  A_eval = A_map p,  q_eval = q_map p  (:433-451).
  * the plugin is called as _CvxpyLayer.apply(P_eval, q_eval, A_eval, ctx, solver_args, needs_grad, warm_start) (:475-483) and
    variables are recovered by slicing primal / dual, Fortran reshape, svec -> symmetric unpacking (:225-282, :144-222).
  * a batch of one is not the same as unbatched: outputs keep the leading axis exactly when an input had it.

What is different (MI355X-first):
  * the parameter maps are evaluated ON THE DEVICE by ce_parammap_apply, batch-major: p is (B, Ptot+1) row-major -- the
    natural layout of the flattened parameters -- and A_eval comes out as (B, nnz_aug) row-major, which is the engine's native
    layout.  The reference's p_stack transpose, its (nnz_aug, B) result and the engine's layout pass all disappear; the plugin
    receives the transposed VIEW (nnz_aug, B) so the boundary convention is unchanged.
  * canonicalisation (host, once) is decoupled: the layer is built from a `CanonTemplate`.  With CVXPY installed,
    `CanonTemplate.from_cvxpy(problem, parameters, variables)` produces it exactly as utils/parse_args.py:388-514 does
    (canonicalising as "DIFFCP"); without CVXPY (this build image) templates are built by hand / by affine probing
    (cvxpylayers_amd.torch.templates).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Any, Sequence

import numpy as np
import scipy.sparse as sp
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd.interfaces import get_solver_ctx, get_torch_cvxpylayer, optimal_value


@dataclass
class VariableRecovery:
    """How one requested variable is cut out of the solver's primal / dual vector (utils/parse_args.py:56-67)."""
    primal: slice | None
    dual: slice | None
    shape: tuple
    source: str = "primal"            # "primal" | "dual"
    unpack_fn: str = "reshape"        # "reshape" | "svec_primal" | "svec_dual"


@dataclass
class CanonTemplate:
    """Everything CVXPY's canonicalisation yields for a DPP problem (host side, built once):
    param_shapes   shapes of the parameters in USER order
    col_offsets    first column of each parameter (user order) in the canonical parameter vector; the constant 1 is last
    A_map          scipy CSR (nnz_aug, Ptot+1): values of the CSC data of [A_cvx | b_cvx] as an affine function of p
    q_map          scipy CSR (n+1, Ptot+1)
    A_structure    (indices, indptr, (m, n+1))  CSC structure of [A_cvx | b_cvx]
    cone_dims      {"z","l","q","ep","s","p"}
    var_recover    one VariableRecovery per requested variable
    """
    param_shapes: list
    col_offsets: list
    A_map: sp.csr_array
    q_map: sp.csr_array
    A_structure: tuple
    cone_dims: dict
    var_recover: list
    P_map: Any = None              # (nnz_P, Ptot+1) map of the quadratic objective 1/2 x^T P x (plugins in SUPPORTS_QUAD_OBJ), or None
    P_structure: Any = None        # (indices, indptr, (n, n)) CSC structure of P (param_prob.reduced_P.problem_data_index)
    gp: bool = False
    gp_log_mask: tuple | None = None
    objective_sign: int = 1        # -1: the problem was a Maximize (the canonical program minimises the negated objective); forward(return_value=True) returns objective_sign * p*

    @property
    def n_params_total(self) -> int:
        return int(self.A_map.shape[1]) - 1

    @staticmethod
    def from_cvxpy(problem, parameters, variables, gp: bool = False):
        """Canonicalise with CVXPY (as "DIFFCP", i.e. SCS cone form and CSC structure).  Needs cvxpy + cvxpylayers."""
        try:
            import cvxpylayers.utils.parse_args as pa  # type: ignore
        except Exception as e:  # pragma: no cover - not installable in the build image
            raise ImportError("CanonTemplate.from_cvxpy needs cvxpy and cvxpylayers; build a template by hand "
                              "(cvxpylayers_amd.torch.templates) when they are not installed") from e
        ctx = pa.parse_args(problem, variables, parameters, "DIFFCP", gp=gp, verbose=False, canon_backend=None, solver_args={})
        sizes = [int(np.prod(p.shape)) if p.shape else 1 for p in parameters]
        order = ctx.user_order_to_col_order
        offs_by_col = np.concatenate([[0], np.cumsum([sizes[list(order).index(k)] for k in range(len(parameters))])])
        col_offsets = [int(offs_by_col[order[i]]) for i in range(len(parameters))]
        rec = [VariableRecovery(v.primal, v.dual, tuple(v.shape), v.source, v.unpack_fn) for v in ctx.var_recover]
        sc = ctx.solver_ctx
        return CanonTemplate([tuple(p.shape) for p in parameters], col_offsets, ctx.reduced_A.reduced_mat.tocsr(), ctx.q.tocsr(),
                             (sc.A_structure[0], sc.A_structure[1], sc.A_shape), dict(sc.dims) if isinstance(sc.dims, dict) else sc.dims,
                             rec, gp=gp, gp_log_mask=ctx.gp_log_mask, objective_sign=-1 if type(problem.objective).__name__ == "Maximize" else 1)


def _reshape_fortran(x: torch.Tensor, shape: tuple) -> torch.Tensor:
    """Column-major reshape (torch/cvxpylayer.py:40-55)."""
    if x.dim() == 0:
        return x.reshape(shape)
    xt = x.permute(*reversed(range(x.dim())))
    return xt.reshape(*reversed(shape)).permute(*reversed(range(len(shape))))


class _DeviceCSR:
    """A scipy CSR matrix and its transpose as int32/fp64 device arrays (lazily per device)."""

    def __init__(self, mat: sp.csr_array):
        self.mat = sp.csr_array(mat).astype(np.float64)
        self.mat.sort_indices()
        self.matT = sp.csr_array(self.mat.T.tocsr())
        self.matT.sort_indices()
        self._dev: dict = {}

    def on(self, device: torch.device):
        key = (device.type, device.index)
        if key not in self._dev:
            def up(m):
                return (torch.from_numpy(m.indptr.astype(np.int32)).to(device), torch.from_numpy(m.indices.astype(np.int32)).to(device),
                        torch.from_numpy(m.data.astype(np.float64)).to(device), int(m.shape[0]))
            self._dev[key] = (up(self.mat), up(self.matT))
        return self._dev[key]


def _spmm_bm(arrs, P: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """out (B, rows) = P (B, cols) . map^T on the device through the C ABI (ce_parammap_apply2); with `out` given, accumulate."""
    indptr, indices, vals, rows = arrs
    B = P.shape[0]
    acc = out is not None
    if out is None:
        out = torch.empty((B, rows), dtype=torch.float64, device=P.device)
    rc = _lib.lib().ce_parammap_apply2(P.device.index or 0, B, rows, P.shape[1], int(acc), indptr.data_ptr(), indices.data_ptr(), vals.data_ptr(),
                                       P.data_ptr(), P.stride(0), out.data_ptr(), out.stride(0),
                                       C.c_void_p(torch.cuda.current_stream(P.device).cuda_stream))
    _lib.check(rc, "ce_parammap_apply2")
    return out


class _ParamMap1(torch.autograd.Function):
    """One map (the quadratic objective's P_eval = P_map p), batch-major, transpose as backward."""

    @staticmethod
    def forward(ctx, csr: _DeviceCSR, p_bm: torch.Tensor):
        fwd, bwd = csr.on(p_bm.device)
        ctx.fwd, ctx.bwd = fwd, bwd
        return _spmm_bm(fwd, p_bm.contiguous())

    @staticmethod
    def jvp(ctx, _, t_p):
        return _spmm_bm(ctx.fwd, t_p.contiguous())      # linear in p (the constant column's tangent is zero)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return None, _spmm_bm(ctx.bwd, g.contiguous())


class _ParamMapApply(torch.autograd.Function):
    """Batch-major evaluation of both parameter maps, (A_bm, q_bm) = (p A_map^T, p q_map^T), with the transposed maps as backward
    accumulated into one p gradient (reference: _ScipySparseMatmul applied once per map, :12-37, and autograd's add)."""

    @staticmethod
    def forward(ctx, A_csr: _DeviceCSR, q_csr: _DeviceCSR, p_bm: torch.Tensor):
        p_bm = p_bm.contiguous()
        fA, bA = A_csr.on(p_bm.device)
        fq, bq = q_csr.on(p_bm.device)
        ctx.fwd, ctx.bwd = (fA, fq), (bA, bq)
        return _spmm_bm(fA, p_bm), _spmm_bm(fq, p_bm)

    @staticmethod
    def jvp(ctx, _A, _q, t_p):
        t_p = t_p.contiguous()                           # both maps are linear in p (the constant column's tangent is zero)
        return _spmm_bm(ctx.fwd[0], t_p), _spmm_bm(ctx.fwd[1], t_p)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gA, gq):
        bA, bq = ctx.bwd
        g = _spmm_bm(bA, gA.contiguous())
        _spmm_bm(bq, gq.contiguous(), out=g)
        return None, None, g


class _ParamGradLayer(torch.autograd.Function):
    """solver_args param_grad="factors": ONE node from the parameter matrix p_bm (B, Ptot+1) to (primal, dual).  Its forward is the two forward parameter maps and
    the plugin forward (what CvxpyLayer.forward chains otherwise); its backward hands the cotangents to interfaces.mi355_if.adjoint_params, which returns the
    gradient of p_bm from the adjoint's factors -- no dA row is written, expanded or read back.  `box` carries what is not a tensor: in {"layer", "solver_args",
    "warm_start", "batch"}, out {"info", "data"}.  A call the engine routes to a path without the mode (a shared A decided from the values) keeps today's
    arithmetic inside the same node: vjp, then the transposed maps."""

    @staticmethod
    def forward(ctx, p_bm: torch.Tensor, box: dict):
        layer = box["layer"]
        p_bm = p_bm.contiguous()
        dev = p_bm.device
        (fA, bA), (fq, bq) = layer._A.on(dev), layer._q.on(dev)
        A_eval, q_eval = _spmm_bm(fA, p_bm).t(), _spmm_bm(fq, p_bm).t()
        if not box["batch"]:
            A_eval, q_eval = A_eval.squeeze(1), q_eval.squeeze(1)
        primal, dual, info, data = get_torch_cvxpylayer(layer.solver).apply(None, q_eval, A_eval, layer.ctx, box["solver_args"], True, box["warm_start"])
        box["info"], box["data"] = info, data
        ctx.box, ctx.bwd = box, (bA, bq)
        ctx.set_materialize_grads(False)
        from cvxpylayers_amd.interfaces.mi355_if import param_grad_served
        ctx.served = param_grad_served(data)
        if not ctx.served:          # (the engine took another path for this call: a shared A decided from the values)
            from cvxpylayers_amd.interfaces.solver_args import _warn_once
            _warn_once("param_grad_unserved", "MI355 solver: solver_args param_grad='factors' is not served on the path this call took; the dA route runs (the key is ignored)")
        if isinstance(info, dict) and isinstance(info.get("adjoint"), dict) and ctx.served:
            info["adjoint"]["param_grad"] = "factors"
        return primal.detach(), dual.detach()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dprimal, ddual):
        from cvxpylayers_amd.interfaces.mi355_if import _ConeLayer, adjoint_params
        box = ctx.box
        data, info, layer = box["data"], box["info"], box["layer"]
        if dprimal is None and ddual is None:
            return None, None
        unbatched = data[2]          # (the plugin returns (1, n), (1, m) for an unbatched call and squeezes dq, dA alone)
        if ctx.served:
            return adjoint_params(data, dprimal, ddual, info, layer._pg_maps()), None
        # not served on this call's path: the plugin's own backward and the transposed maps, as the default route computes them
        shim = type("Shim", (), {})()
        shim.backward_data, shim.info = data, info
        _dP, dq, dA, *_ = _ConeLayer.backward(shim, dprimal, ddual, None, None)
        if unbatched:
            dq, dA = dq.unsqueeze(1), dA.unsqueeze(1)
        bA, bq = ctx.bwd
        with torch.cuda.device(dA.device):
            g = _spmm_bm(bA, dA.t().contiguous())
            _spmm_bm(bq, dq.t().contiguous(), out=g)
        return g, None


def _svec_to_symmetric(svec, k, batch, rows, cols, scale=None):
    rows_t = torch.as_tensor(rows, dtype=torch.long, device=svec.device)
    cols_t = torch.as_tensor(cols, dtype=torch.long, device=svec.device)
    data = svec * torch.as_tensor(scale, dtype=svec.dtype, device=svec.device) if scale is not None else svec
    out = torch.zeros(batch + (k, k), dtype=svec.dtype, device=svec.device)
    out[..., rows_t, cols_t] = data
    out[..., cols_t, rows_t] = data
    return out


def _unpack_primal_svec(svec, k, batch):
    """Symmetric primal variable: upper triangle, row-major, unscaled (torch/cvxpylayer.py:183-198)."""
    rows, cols = np.triu_indices(k)
    return _svec_to_symmetric(svec, k, batch, rows, cols)


def _unpack_svec(svec, k, batch):
    """PSD dual: lower triangle, column-major, off-diagonals scaled by sqrt(2) (torch/cvxpylayer.py:201-222)."""
    rr, cc = np.tril_indices(k)
    order = np.lexsort((rr, cc))
    rows, cols = rr[order], cc[order]
    return _svec_to_symmetric(svec, k, batch, rows, cols, np.where(rows == cols, 1.0, 1.0 / np.sqrt(2.0)))


def _recovery_map(var_recover, n_src: int, source: str):
    """The variable recovery of one source (primal or dual) as a sparse map R (sum of output sizes x n_src): output element t of a
    variable, in the row-major order of its final shape, is scale * src[index].  Slices + Fortran reshapes give one entry per row;
    svec unpacking gives the 1 (primal) or 1/sqrt(2) off-diagonal (PSD dual) weights of torch/cvxpylayer.py:183-222.  Returns
    (csr, [(variable position, row offset, size)])."""
    rows, cols, vals, layout, off = [], [], [], [], 0
    for pos, var in enumerate(var_recover):
        if var.source != source:
            continue
        sl = var.primal if source == "primal" else var.dual
        src = np.arange(n_src)[sl]
        shape = tuple(var.shape)
        size = int(np.prod(shape)) if len(shape) else 1
        if var.unpack_fn == "reshape":
            # out.reshape(-1)[t] = data[f(t)] with data Fortran-ordered over `shape`
            idx = np.arange(size).reshape(shape, order="F").reshape(-1) if len(shape) > 1 else np.arange(size)
            rows.append(off + np.arange(size)); cols.append(src[idx]); vals.append(np.ones(size))
        elif var.unpack_fn in ("svec_primal", "svec_dual"):
            k = shape[0]
            if var.unpack_fn == "svec_primal":
                rr, cc = np.triu_indices(k)
                w = np.ones(rr.size)
            else:
                r0, c0 = np.tril_indices(k)
                order = np.lexsort((r0, c0))
                rr, cc = r0[order], c0[order]
                w = np.where(rr == cc, 1.0, 1.0 / np.sqrt(2.0))
            rows.append(off + rr * k + cc); cols.append(src); vals.append(w)
            offd = rr != cc
            rows.append(off + cc[offd] * k + rr[offd]); cols.append(src[offd]); vals.append(w[offd])
        else:
            raise ValueError(f"Unknown variable recovery type: {var.unpack_fn}")
        layout.append((pos, off, size))
        off += size
    if not layout:
        return None, []
    mat = sp.csr_array((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(off, n_src))
    return mat, layout


class _RecoverMap(torch.autograd.Function):
    """Variable recovery of one source as ONE launch of the sparse-map kernel (ce_parammap_apply2) writing every requested variable
    in its final layout, and its transpose as the backward (gradients of all variables gathered into d primal / d dual in one
    launch).  Replaces the per-variable slice / permute / index_put chain of _recover_results_torch, which stays as the checker."""

    @staticmethod
    def forward(ctx, csr: _DeviceCSR, layout, shapes, src: torch.Tensor):
        fwd, bwd = csr.on(src.device)
        ctx.fwd, ctx.bwd, ctx.layout, ctx.shapes, ctx.total, ctx.src_shape = fwd, bwd, layout, shapes, fwd[3], src.shape
        return _RecoverMap._recover(fwd, layout, shapes, src)

    @staticmethod
    def _recover(fwd, layout, shapes, src):
        src2 = src.reshape(-1, src.shape[-1]).contiguous()
        with torch.cuda.device(src.device):
            rec = _spmm_bm(fwd, src2)
        lead = tuple(src.shape[:-1])
        return tuple(rec[:, off:off + size].reshape(lead + tuple(shape)) if len(layout) > 1 else rec.reshape(lead + tuple(shape))
                     for (_, off, size), shape in zip(layout, shapes))

    @staticmethod
    def jvp(ctx, _csr, _layout, _shapes, t_src):
        return _RecoverMap._recover(ctx.fwd, ctx.layout, ctx.shapes, t_src)      # the recovery is linear

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        B = int(np.prod(ctx.src_shape[:-1])) if len(ctx.src_shape) > 1 else 1
        ref = next(g for g in grads if g is not None)
        parts = [g.reshape(B, size) if g is not None else torch.zeros((B, size), dtype=ref.dtype, device=ref.device)
                 for g, (_, _, size) in zip(grads, ctx.layout)]
        g_rec = parts[0].contiguous() if len(parts) == 1 else torch.cat(parts, dim=1)
        with torch.cuda.device(ref.device):
            d_src = _spmm_bm(ctx.bwd, g_rec)
        return None, None, None, d_src.reshape(ctx.src_shape)


class _Ctx:
    """The object handed to the plugin as cl_ctx (the plugin only needs .solver_ctx)."""

    def __init__(self, solver_ctx, solver):
        self.solver_ctx = solver_ctx
        self.solver = solver


class _ParamProbView:
    """Minimal stand-in for CVXPY's ParamConeProg as far as interfaces.get_solver_ctx reads it."""

    class _Red:
        def __init__(self, pdi, mat=None):
            self.problem_data_index = pdi
            self.reduced_mat = mat          # the parameter map (ParamConeProg.reduced_A.reduced_mat): lets the plugin decide structurally whether A is batch-invariant

    def __init__(self, a_structure, p_structure=None, a_map=None):
        self.reduced_A = self._Red(a_structure, a_map)
        self.reduced_P = self._Red(p_structure) if p_structure is not None else None


class CvxpyLayer(torch.nn.Module):
    """Differentiable cone-program layer on MI355X.

    CvxpyLayer(problem, parameters, variables, solver="MI355", gp=False, solver_args=None)   # needs cvxpy
    CvxpyLayer(template=CanonTemplate(...), solver_args=None)                                # cvxpy-free
    """

    def __init__(self, problem=None, parameters: Sequence | None = None, variables: Sequence | None = None, solver: str | None = None,
                 gp: bool = False, verbose: bool = False, canon_backend=None, solver_args: dict | None = None,
                 template: CanonTemplate | None = None):
        super().__init__()
        if template is None:
            if problem is None:
                raise ValueError("CvxpyLayer needs either a CVXPY problem or a CanonTemplate")
            template = CanonTemplate.from_cvxpy(problem, parameters, variables, gp=gp)
        solver = solver or "MI355"
        if solver != "MI355":
            raise RuntimeError("Unknown solver. Check if your solver is supported by CVXPYlayers")
        if template.objective_sign not in (1, -1):
            raise ValueError(f"CanonTemplate.objective_sign must be 1 or -1, got {template.objective_sign!r}")
        self.template = template
        self.solver = solver
        opts = dict(solver_args or {})
        solver_ctx = get_solver_ctx(solver, _ParamProbView(template.A_structure, template.P_structure if template.P_map is not None else None, template.A_map),
                                    template.cone_dims, {}, opts, verbose)
        self.ctx = _Ctx(solver_ctx, solver)
        # The maps address parameters Fortran-flattened (the reference's p_stack); the device copies are re-indexed once to the
        # parameters' native row-major layout so flattening a batched parameter is a contiguous copy, not a strided transpose.
        colmap = np.arange(template.n_params_total + 1)
        for shape, off in zip(template.param_shapes, template.col_offsets):
            size = int(np.prod(shape)) if len(shape) else 1
            if len(shape) > 1:
                colmap[off:off + size] = off + np.arange(size).reshape(shape).reshape(-1, order="F")
        inv = np.empty_like(colmap)
        inv[colmap] = np.arange(colmap.size)

        def recol(mat):
            # new column c holds the parameter entry that was at Fortran column f: new = old[:, f(c)], with f(c) = position of c in colmap
            return sp.csr_array(sp.csr_array(mat)[:, inv])
        self._A = _DeviceCSR(recol(template.A_map))
        self._q = _DeviceCSR(recol(template.q_map))
        self._P = _DeviceCSR(recol(template.P_map)) if template.P_map is not None else None
        self.batch_sizes: list | None = None
        # variable recovery as one sparse-map launch per source (and its transpose in backward); CE_FUSED_RECOVERY=0 keeps the
        # per-variable torch chain (the checker of tests/test_gpu_recovery.py)
        n_primal = int(template.q_map.shape[0]) - 1
        n_dual = int(template.A_structure[2][0])
        self._rec = {}
        for source, n_src in (("primal", n_primal), ("dual", n_dual)):
            mat, layout = _recovery_map(template.var_recover, n_src, source)
            if mat is not None:
                self._rec[source] = (_DeviceCSR(mat), layout)
        self.fused_recovery = os.environ.get("CE_FUSED_RECOVERY", "1") != "0"
        self._pg = None          # (_pg_maps)

    def _pg_maps(self):
        """the layer's transposed parameter maps composed for k_param_grad (interfaces/param_grad.py), built on first use.  The row of the constant column is left
        empty: the layer never reads that column of g (jacobian slices by col_offsets, the ones column of p_bm has no gradient), yet it holds every constant entry
        of A.  A native QP's transposed P map goes in with P's structure: the one-triangle doubling, or the transpose of the plugin's symmetrisation of a full
        structure, in the values."""
        if self._pg is None:
            from cvxpylayers_amd.interfaces.param_grad import ComposedMaps
            tpl = self.template
            own = lambda matT: sp.vstack([sp.csr_array(matT)[:-1], sp.csr_array((1, matT.shape[1]))], format="csr")          # (the constant column's row, emptied)
            p_args = ()
            quad = getattr(self.ctx.solver_ctx, "quad", None)
            if self._P is not None and quad is not None and quad.sym_perm is not None:
                p_args = (own(self._P.matT), quad.p_rows, quad.p_cols, quad.one_triangle, None if quad.one_triangle else quad.sym_perm)
            self._pg = ComposedMaps(own(self._A.matT), own(self._q.matT), tpl.A_structure[0], tpl.A_structure[1], int(tpl.q_map.shape[0]) - 1, int(tpl.A_structure[2][0]), *p_args)
        return self._pg

    def _param_grad_route(self, merged: dict, device, forward_ad: bool = False, many: bool = False) -> bool:
        """solver_args param_grad == "factors" AND this layer is served on `device` as far as the template and the arguments decide it (the engine's path of a
        call -- a shared A -- is known only behind the solve).  many: the call makes many-cotangent calls (jacobian in the reverse direction), where a native QP,
        exponential / power cones and PSD blocks are served under their own key (qp_adjoint / tri_adjoint / psd_adjoint = "search_free"); one cotangent
        (.backward(), forward-mode AD) belongs to the pivoting kernels there, as those keys say.  Not served: one notice, the dA route."""
        from cvxpylayers_amd import _lib
        from cvxpylayers_amd.interfaces.solver_args import _warn_once, adjoint_mode, lpgd_rule, param_grad, psd_adjoint, qp_adjoint, tri_adjoint
        if param_grad(merged) != "factors":
            return False
        why = None
        eng = None if self.template.gp else self.ctx.solver_ctx.engine(device)
        h = None if eng is None else eng._h
        L = _lib.lib()
        if self.template.gp:
            why = "a quadratic objective or a gp=True layer"
        elif adjoint_mode(merged) != "direct" or lpgd_rule(merged) is not None:
            why = f"solver_args mode={merged.get('mode')!r}"
        elif forward_ad:
            why = "forward-mode AD"
        elif self._P is not None:
            if qp_adjoint(merged) != "search_free" or L.ce_vjp_qp_many_variant(h) < 0:
                why = "a quadratic objective or a gp=True layer"
            elif not many:
                why = "one cotangent through a quadratic objective (qp_adjoint='search_free' serves jacobian(direction='reverse') alone)"
        elif eng.param_grad_variant < 0:
            tri = tri_adjoint(merged) == "search_free" and L.ce_vjp_tri_many_variant(h) >= 0
            psd = psd_adjoint(merged) == "search_free" and (L.ce_vjp_psd_many_variant(h) >= 0 or L.ce_vjp_psd_tri_many_variant(h) >= 0)
            if not (tri or psd):
                why = "this template (PSD / exponential / power cones without tri_adjoint / psd_adjoint='search_free', n > 108, or CE_BWD_NS=0)"
            elif not many:
                why = "one cotangent on this template (tri_adjoint / psd_adjoint='search_free' serve jacobian(direction='reverse') alone)"
        if why is None:
            return True
        _warn_once("param_grad_unserved", f"MI355 solver: solver_args param_grad='factors' is not served for {why}; the dA route runs (the key is ignored)")
        return False

    # ---- utils/parse_args.py:94-143
    def validate_params(self, values: list) -> tuple:
        shapes = self.template.param_shapes
        if len(values) != len(shapes):
            raise ValueError("A tensor must be provided for each CVXPY parameter; "
                             f"received {len(values)} tensors, expected {len(shapes)}")
        batch_sizes = []
        for i, (value, shape) in enumerate(zip(values, shapes)):
            shape = tuple(shape)
            if value.dim() == len(shape):
                if tuple(value.shape) != shape:
                    raise ValueError(f"Invalid parameter shape for parameter {i}. Expected: {shape}, Got: {tuple(value.shape)}")
                batch_sizes.append(0)
            elif value.dim() == len(shape) + 1:
                if tuple(value.shape[1:]) != shape:
                    raise ValueError(f"Invalid parameter shape for parameter {i}. Expected batched shape: "
                                     f"(batch_size, {', '.join(map(str, shape))}), Got: {tuple(value.shape)}")
                batch_sizes.append(int(value.shape[0]))
            else:
                raise ValueError(f"Invalid parameter dimensionality for parameter {i}. Expected {len(shape)} or "
                                 f"{len(shape) + 1} dimensions, Got: {value.dim()} dimensions")
        nonzero = [b for b in batch_sizes if b > 0]
        self.batch_sizes = batch_sizes
        if nonzero:
            if not all(b == nonzero[0] for b in nonzero):
                raise ValueError("Inconsistent batch sizes. Expected all batched parameters to have the same batch size, "
                                 f"but got: {batch_sizes}")
            return (nonzero[0],)
        return ()

    def _flatten_params(self, params, batch) -> torch.Tensor:
        """(B, Ptot+1) row-major parameter matrix: flattened parameters at their canonical column ranges, then the constant 1
        (the batch-major transpose of the reference's p_stack, torch/cvxpylayer.py:84-141)."""
        B = batch[0] if batch else 1
        dev = params[0].device
        tot = self.template.n_params_total
        flats = []
        for i, value in enumerate(params):
            v = value.to(torch.float64)
            if self.batch_sizes[i] == 0:
                v = v.unsqueeze(0).expand((B,) + tuple(v.shape))
            flats.append(v.reshape(B, -1))                       # row-major; the device maps were re-indexed to match (__init__)
        order = sorted(range(len(flats)), key=lambda i: self.template.col_offsets[i])
        pos, tiled = 0, True
        for i in order:
            tiled = tiled and self.template.col_offsets[i] == pos
            pos += flats[i].shape[1]
        if tiled and pos == tot:
            # one concatenation: its backward hands each parameter a view of the gradient (in-place slice writes would make autograd
            # clone the whole (B, Ptot+1) gradient once per parameter)
            return torch.cat([flats[i] for i in order] + [torch.ones((B, 1), dtype=torch.float64, device=dev)], dim=1)
        p = torch.zeros((B, tot + 1), dtype=torch.float64, device=dev)
        p[:, tot] = 1.0
        for i, flat in enumerate(flats):
            off = self.template.col_offsets[i]
            p[:, off:off + flat.shape[1]] = flat
        return p

    def forward(self, *params: torch.Tensor, solver_args: dict | None = None, warm_start: bool = False, return_value: bool = False):
        """return_value=True appends the optimal value of the problem as the LAST output: (B,) float64, or () when no parameter is batched; its gradients are the
        envelope theorem's (interfaces/optimal_value.py: no adjoint system is solved for them).  gp=True layers return exp(value) (the log-problem's objective is the
        log of the original's), Maximize problems the maximum (template.objective_sign).  info["objective"] holds the canonical program's primal and dual objective."""
        if not isinstance(return_value, bool):
            raise TypeError(f"return_value must be a bool, got {type(return_value).__name__}")
        solver_args = solver_args or {}
        from cvxpylayers_amd.interfaces.solver_args import param_grad
        merged = {**self.ctx.solver_ctx.options, **solver_args}
        want_factors = param_grad(merged) == "factors"          # (a wrong value raises here, before the device is touched)
        batch = self.validate_params(list(params))
        if self.template.gp and self.template.gp_log_mask is not None:
            params = tuple(torch.log(p) if lg else p for p, lg in zip(params, self.template.gp_log_mask))
        if params[0].device.type != "cuda":
            raise RuntimeError("MI355 solver needs parameters on a ROCm device; there is no CPU fallback (use solver='DIFFCP' on CPU)")
        with torch.cuda.device(params[0].device):
            p_bm = self._flatten_params(params, batch)
            has_tan = want_factors and any(torch.autograd.forward_ad.unpack_dual(p).tangent is not None for p in params)
            if want_factors and ((torch.is_grad_enabled() and p_bm.requires_grad) or has_tan):
                if self._param_grad_route(merged, params[0].device, forward_ad=has_tan):
                    return self._forward_param_grad(p_bm, params, batch, solver_args, warm_start, return_value)
            A_bm, q_bm = _ParamMapApply.apply(self._A, self._q, p_bm)   # (B, nnz_aug) engine-native, (B, n+1)
            P_eval = _ParamMap1.apply(self._P, p_bm).t() if self._P is not None else None
        A_eval, q_eval = A_bm.t(), q_bm.t()                     # the reference's (nnz_aug, B) / (n+1, B), as views
        if not batch:
            A_eval, q_eval = A_eval.squeeze(1), q_eval.squeeze(1)
            P_eval = P_eval.squeeze(1) if P_eval is not None else None
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        if not needs_grad:          # forward-mode AD (torch.autograd.forward_ad): a parameter that carries a tangent needs the same saved state
            needs_grad = any(torch.autograd.forward_ad.unpack_dual(p).tangent is not None for p in params)
        layer_cls = get_torch_cvxpylayer(self.solver)
        # warm_start=True: the plugin starts from this layer's previous solution when the batch size matches (the reference keeps
        # the same cache for its MOREAU plugin, torch/cvxpylayer.py:464-487)
        primal, dual, info, _ = layer_cls.apply(P_eval, q_eval, A_eval, self.ctx, solver_args, needs_grad, True if warm_start else None)
        self.info = info
        out = self._recover_results(primal, dual, batch) if self.fused_recovery else self._recover_results_torch(primal, dual, batch)
        if return_value:
            out = out + (self._value(P_eval, q_eval, A_eval, primal, dual, info, solver_args),)
        return out

    def _forward_param_grad(self, p_bm, params, batch, solver_args, warm_start, return_value):
        """forward under solver_args param_grad="factors" on a served layer: one autograd node from p_bm to (primal, dual) (_ParamGradLayer)"""
        box = {"layer": self, "solver_args": solver_args, "warm_start": True if warm_start else None, "batch": batch}
        primal, dual = _ParamGradLayer.apply(p_bm, box)
        info = box["info"]
        self.info = info
        out = self._recover_results(primal, dual, batch) if self.fused_recovery else self._recover_results_torch(primal, dual, batch)
        if return_value:          # (the value's envelope gradients flow through A_eval / q_eval themselves: the forward maps once more, with their graph)
            A_bm, q_bm = _ParamMapApply.apply(self._A, self._q, p_bm)
            A_eval, q_eval = A_bm.t(), q_bm.t()
            if not batch:
                A_eval, q_eval = A_eval.squeeze(1), q_eval.squeeze(1)
            out = out + (self._value(None, q_eval, A_eval, primal, dual, info, solver_args),)
        return out

    def jacobian(self, *params: torch.Tensor, solver_args: dict | None = None, max_bytes: int = 1 << 30, direction: str = "reverse"):
        """outs, jac = layer.jacobian(*params): `outs` is what forward returns, detached; jac[i][j] = d outs[i] / d params[j] per instance, of shape
        batch + var_i.shape + param_j.shape (both index groups in torch's row-major order), float64, on the parameters' device.  A parameter passed unbatched into a
        batched call is differentiated per instance (its expanded copy), not summed over the batch.

        No autograd graph anywhere: one plugin forward, then one cotangent per output element (the rows of the transposed recovery maps, the same for every instance)
        through interfaces.mi355_if.adjoint_many -- ConeEngine.vjp_many: each instance is factored once per chunk, not once per output element -- and the transposed
        parameter maps on the (K B, .) views.  The cotangents go in chunks whose dA stays within max_bytes (K_chunk B nnz_aug 8 bytes, at least one cotangent); a
        cotangent's result does not depend on the chunk it travels in.  Instances a raise_on_error=False call masks return NaN rows, like their outputs.
        A quadratic objective inside the kernels runs the loop of K ce_vjp_qp calls here by default; solver_args {"qp_adjoint": "search_free"} makes one
        ce_vjp_qp_many call per chunk instead (the search-free elimination with P factors each instance once and returns dP too; a chunk's dP then counts against
        max_bytes beside its dA; info["adjoint"]["path"] == "ce_vjp_qp_many").  Opt-in: a rank-deficient instance keeps that route's dropped-variable answer with
        status 4.  The single-cotangent backward of .backward() ignores the key.
        A template with exponential / power cones runs the loop of K ce_vjp calls (the pivoting kernel) here by default; solver_args {"tri_adjoint": "search_free"}
        makes one ce_vjp_tri_many call per chunk instead (the search-free elimination diagonalises and rotates each triple and factors each instance once for the
        chunk; chunking by max_bytes is unchanged; info["adjoint"]["path"] == "ce_vjp_tri_many").  Opt-in: the two kernels need not flag the same instances (a pivot
        search there; here a weighted triple row with 1 - lambda < 1e-5 flags too), and a flagged instance gets LSQR's minimum-norm answer.  .backward() ignores
        the key; direction="forward" and "auto" keep their rules (the forward direction has a key of its own, below).
        A template with PSD blocks runs the loop of K ce_vjp calls (the pivoting kernel, the blocks' decompositions with it) here by default; solver_args
        {"psd_adjoint": "search_free"} makes one ce_vjp_psd_many call per chunk instead (each block decomposed, its rows rotated and each instance factored once for
        the chunk; chunking by max_bytes is unchanged; info["adjoint"]["path"] == "ce_vjp_psd_many").  Opt-in for the triples' reason, with the triples' stiff-row
        rule carried over to PSD rows; independent of psd_elimination; .backward() ignores the key.  With exponential / power cones beside the blocks the one call
        is ce_vjp_psd_tri_many (tri_adjoint stays inert there).
        Refused (NotImplementedError): gp=True layers, a quadratic objective that reaches the engine as a torch-op epigraph, solver_args `mode` of the LPGD family.

        direction="forward": the Jacobian by COLUMNS -- one plugin forward, then one tangent per parameter entry (the columns of the forward parameter maps of A, q
        and P, the same for every instance: handed over once, batch stride 0; the constant column is left out) through interfaces.mi355_if.tangent_many --
        ConeEngine.jvp_many --, in chunks whose dx, dy stay within max_bytes, and the recovery maps on dx / dy.  Same return, same layout.  The route for a layer
        with few parameter entries and many output elements, and the one by which a quadratic objective inside the kernels gets a one-factorisation Jacobian.
        It runs the direct elimination unless solver_args (the call's or the layer's) says jvp_mode="lsqr" explicitly: a Jacobian by K LSQR solves is not a
        default anyone wants.  A template with exponential / power cones runs the loop of K ce_jvp calls here by default (every triple diagonalised, its rows
        rotated and every instance factored once per parameter entry); solver_args {"tri_tangents": "many"} makes one ce_jvp_tri_many call per chunk instead: all
        of that once per instance for the chunk, and one LSQR launch for the flagged instances of every tangent (info["jvp"]["kernel"] == "ce_jvp_tri_many",
        info["jvp"]["path"] stays "direct"; chunking is unchanged).  Opt-in; forward-mode AD with one tangent ignores the key.  A template with PSD blocks runs K single-tangent calls
        here by default (ce_jvp_lsqr, under psd_elimination="search_free" too); solver_args {"psd_tangents": "many"} makes one ce_jvp_psd_many call per chunk instead
        (info["jvp"]["kernel"] == "ce_jvp_psd_many", info["jvp"]["path"] "direct"; chunking is unchanged).  Opt-in; one-tangent forward-mode AD ignores the key.
        With exponential / power cones beside the blocks the one call is ce_jvp_psd_tri_many (tri_tangents stays inert there).
        direction="auto": forward when the parameter entries are fewer than the output elements, reverse otherwise.  (Named `direction`
        because solver_args["mode"] means something else.)  Any other value: ValueError, before anything touches the device."""
        from cvxpylayers_amd.interfaces.mi355_if import adjoint_many, adjoint_many_params, param_grad_served, tangent_many
        from cvxpylayers_amd.interfaces.solver_args import LPGD_MODES, _warn_once, param_grad
        if direction not in ("reverse", "forward", "auto"):
            raise ValueError(f"CvxpyLayer.jacobian: direction must be 'reverse', 'forward' or 'auto', got {direction!r}")
        solver_args = solver_args or {}
        if self.template.gp:
            raise NotImplementedError("CvxpyLayer.jacobian: gp=True layers are not served (the log / exp maps around the cone program are outside the Jacobian assembled here)")
        merged = {**self.ctx.solver_ctx.options, **solver_args}
        want_factors = param_grad(merged) == "factors"          # (a wrong value raises here, before the device is touched)
        if merged.get("mode") in LPGD_MODES:
            raise NotImplementedError(f"CvxpyLayer.jacobian: solver_args mode={merged.get('mode')!r} has no Jacobian: the LPGD gradient is not linear in the cotangent")
        if int(max_bytes) <= 0:
            raise ValueError(f"max_bytes must be positive, got {max_bytes!r}")
        batch = self.validate_params(list(params))
        if params[0].device.type != "cuda":
            raise RuntimeError("MI355 solver needs parameters on a ROCm device; there is no CPU fallback (use solver='DIFFCP' on CPU)")
        dev = params[0].device
        tpl = self.template
        with torch.no_grad(), torch.cuda.device(dev):
            p_bm = self._flatten_params([p.detach() for p in params], batch).contiguous()
            (fA, bA), (fq, bq) = self._A.on(dev), self._q.on(dev)
            A_bm, q_bm = _spmm_bm(fA, p_bm), _spmm_bm(fq, p_bm)
            P_eval = _spmm_bm(self._P.on(dev)[0], p_bm).t() if self._P is not None else None
            A_eval, q_eval = A_bm.t(), q_bm.t()
            if not batch:
                A_eval, q_eval = A_eval.squeeze(1), q_eval.squeeze(1)
                P_eval = P_eval.squeeze(1) if P_eval is not None else None
            primal, dual, info, data = get_torch_cvxpylayer(self.solver).apply(P_eval, q_eval, A_eval, self.ctx, solver_args, True, None)
            self.info = info
            saved = data[0]
            if self._P is not None and saved.P_bm is None:
                raise NotImplementedError("CvxpyLayer.jacobian: this quadratic objective reaches the engine as a torch-op epigraph (QuadEpigraph), whose derivative "
                                          "lives in autograd; only a quadratic objective inside the kernels is served")
            outs = self._recover_results(primal, dual, batch) if self.fused_recovery else self._recover_results_torch(primal, dual, batch)
            B = batch[0] if batch else 1
            eng = saved.eng
            sizes = [int(np.prod(s)) if len(s) else 1 for s in tpl.param_shapes]
            k_chunk = max(1, int(max_bytes) // max(1, B * eng.nnz_aug * 8))
            if saved.P_bm is not None and saved.qp_adjoint == "search_free":          # (one ce_vjp_qp_many call per chunk: its dP (K_chunk, B, nnz_p) counts beside its dA)
                k_chunk = max(1, int(max_bytes) // max(1, B * (eng.nnz_aug + eng.nnz_p) * 8))
            n_out = sum(int(self._rec[src][0].mat.shape[0]) for src in self._rec)
            forward = direction == "forward" or (direction == "auto" and tpl.n_params_total < n_out)
            # solver_args param_grad="factors", reverse direction: one adjoint_many_params call per chunk straight into g_all[t0:t1] -- no dA; a chunk holds its
            # factor records and dq, B ((m + 1 + n) + (n + 1)) 8 bytes per cotangent (the records keep r_x beside r_y and r_tau), g_all is the result itself.  The
            # same for a native QP, exponential / power cones and PSD blocks under their own many-cotangent key (no dP is counted: none is written)
            factors = want_factors and not forward and self._param_grad_route(merged, dev, many=True)
            if factors and not param_grad_served(data, many=True):          # (the engine took another path for this call: a shared A decided from the values)
                _warn_once("param_grad_unserved", "MI355 solver: solver_args param_grad='factors' is not served on the path this call took; the dA route runs (the key is ignored)")
                factors = False
            if factors:
                k_chunk = max(1, int(max_bytes) // max(1, B * ((eng.m + 1 + eng.n) + (eng.n + 1)) * 8))
            sym_perm = None
            if saved.P_bm is not None and not self.ctx.solver_ctx.quad.one_triangle:          # (the plugin symmetrises P_eval in front of the kernels: its transpose here)
                sym_perm = torch.from_numpy(self.ctx.solver_ctx.quad.sym_perm).to(eng.device)
            jac: list = [None] * len(tpl.var_recover)
            g_fwd = {}
            if forward:
                # one tangent per parameter entry: column c of the forward maps, batch-shared; dx, dy (and ds inside the engine) of a chunk stay within max_bytes
                ptot = tpl.n_params_total
                method = "lsqr" if merged.get("jvp_mode") == "lsqr" else "direct"
                c_chunk = max(1, int(max_bytes) // max(1, B * (eng.n + 2 * eng.m) * 8))
                g_fwd = {src: torch.zeros((int(self._rec[src][0].mat.shape[0]), B, ptot + 1), dtype=torch.float64, device=eng.device) for src in self._rec}
                for c0 in range(0, ptot, c_chunk):
                    c1 = min(ptot, c0 + c_chunk)
                    def cols(dcsr):
                        return torch.from_numpy(np.ascontiguousarray(dcsr.mat[:, c0:c1].toarray().T)).to(eng.device)
                    dx, dy, _failed = tangent_many(data, cols(self._P) if saved.P_bm is not None else None, cols(self._q), cols(self._A), info, method=method, sym_perm=sym_perm)
                    for src, d in (("primal", dx), ("dual", dy)):
                        if src in self._rec:
                            rec = _spmm_bm(self._rec[src][0].on(eng.device)[0], d.view((c1 - c0) * B, -1))          # (K B, outputs) = d . recovery^T
                            g_fwd[src][:, :, c0:c1] = rec.view(c1 - c0, B, -1).permute(2, 1, 0)
            for source in ("primal", "dual"):
                if source not in self._rec:
                    continue
                csr, layout = self._rec[source]
                total = int(csr.mat.shape[0])
                g_all = g_fwd[source] if forward else torch.empty((total, B, tpl.n_params_total + 1), dtype=torch.float64, device=eng.device)
                for t0 in (() if forward else range(0, total, k_chunk)):          # (the reverse direction: rows of the Jacobian, as before)
                    t1 = min(total, t0 + k_chunk)
                    rows = torch.from_numpy(csr.mat[t0:t1].toarray()).to(eng.device)          # one cotangent per output element: a row of the recovery map
                    cot = rows[:, None, :].expand(t1 - t0, B, rows.shape[1]).contiguous()
                    if factors:
                        adjoint_many_params(data, cot if source == "primal" else None, cot if source == "dual" else None, info, self._pg_maps(), out=g_all[t0:t1])
                        continue
                    dA, dq, dP, failed = adjoint_many(data, cot if source == "primal" else None, cot if source == "dual" else None, info)
                    g = g_all[t0:t1].view((t1 - t0) * B, -1)
                    _spmm_bm(bA, dA.view((t1 - t0) * B, -1), out=g.zero_())
                    _spmm_bm(bq, dq.view((t1 - t0) * B, -1), out=g)
                    if dP is not None:
                        if sym_perm is not None:
                            dP = 0.5 * (dP + dP.index_select(2, sym_perm))
                        _spmm_bm(self._P.on(dev)[1], dP.contiguous().view((t1 - t0) * B, -1), out=g)
                if saved.failed is not None:
                    g_all = torch.where(saved.failed[None, :, None], float("nan"), g_all)
                for pos, off, size in layout:
                    vshape = tuple(tpl.var_recover[pos].shape)
                    jac[pos] = tuple(g_all[off:off + size, :, po:po + ps].permute(1, 0, 2).reshape(batch + vshape + tuple(pshape)).to(dev)
                                     for po, ps, pshape in zip(tpl.col_offsets, sizes, tpl.param_shapes))
        return tuple(o.detach() for o in outs), tuple(jac)

    def _value(self, P_eval, q_eval, A_eval, primal, dual, info, solver_args):
        """the optimal value behind the plugin call (see forward): masked instances of a raise_on_error=False call are NaN and contribute no gradient"""
        merged = {**self.ctx.solver_ctx.options, **solver_args}
        status = info.get("status") if isinstance(info, dict) else None
        failed = (status < 0) if (not bool(merged.get("raise_on_error", True)) and status is not None and status.numel()) else None
        val = optimal_value(P_eval, q_eval, A_eval, primal, dual, self.ctx, failed=failed, info=info if isinstance(info, dict) else None)
        if self.template.objective_sign == -1:
            val = -val
        return torch.exp(val) if self.template.gp else val

    def _recover_results(self, primal, dual, batch):
        """torch/cvxpylayer.py:225-282 as one map launch per source (see _RecoverMap)."""
        out = [None] * len(self.template.var_recover)
        for source, src in (("primal", primal), ("dual", dual)):
            if source not in self._rec:
                continue
            csr, layout = self._rec[source]
            shapes = [tuple(self.template.var_recover[pos].shape) for pos, _, _ in layout]
            res = _RecoverMap.apply(csr, layout, shapes, src)
            for (pos, _, _), r in zip(layout, res):
                r = r.reshape(batch + tuple(self.template.var_recover[pos].shape))
                if self.template.gp and source == "primal":
                    r = torch.exp(r)
                out[pos] = r
        return tuple(out)

    # ---- torch/cvxpylayer.py:225-282, per variable with torch ops (checker of the fused path)
    def _recover_results_torch(self, primal, dual, batch):
        internal = tuple(primal.shape[:-1])
        out = []
        for var in self.template.var_recover:
            data = primal[..., var.primal] if var.source == "primal" else dual[..., var.dual]
            if var.unpack_fn == "svec_primal":
                res = _unpack_primal_svec(data, var.shape[0], internal)
            elif var.unpack_fn == "svec_dual":
                res = _unpack_svec(data, var.shape[0], internal)
            elif var.unpack_fn == "reshape":
                res = _reshape_fortran(data, internal + tuple(var.shape))
            else:
                raise ValueError(f"Unknown variable recovery type: {var.unpack_fn}")
            res = res.reshape(batch + tuple(var.shape))
            if self.template.gp and var.source == "primal":
                res = torch.exp(res)
            out.append(res)
        return tuple(out)

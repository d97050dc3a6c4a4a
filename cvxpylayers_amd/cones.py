"""Differentiable Euclidean projections onto products of cones (diffcp's cones.pi / cones.dpi on the GPU).

    project(v, cones, dual=False)      Pi_K(v), or Pi_K*(v), of v (..., m); differentiable in reverse and forward mode
    ConeProjection(cones, dual=False)  the same operation as a torch.nn.Module
    svec(X), smat(v, k), project_psd(X)   PSD blocks as symmetric matrices

`cones` is the dict used everywhere in this package, {"z", "l", "q": [...], "s": [...], "ep", "p": [...]}, rows in the solver's order z, l, q, s, ep, p; a PSD block is
its svec (lower triangle, column-major, sqrt(2) off-diagonals); a negative power-cone entry -a is the dual power cone of exponent a.  The zero cone projects to 0
and its dual is free; every other dual is the true dual cone.

The arithmetic is float64 on the device (include/cone_engine.h ce_cone_project / ce_cone_dproject: one launch per cone kind present); the result comes back in v's
dtype on v's device.  D Pi(v) is symmetric for every cone kind, so the reverse and the forward mode are the same kernel call g -> D Pi(v) g.  Conventions at
kinks are the oracle's: factor 1/2 for a nonnegative row at exactly 0; the identity on a second-order cone's boundary and 0 on its polar's; PSD divided
differences 1 for two positive eigenvalues and 0 for two non-positive ones.  Double backward is not offered.  A non-finite entry makes the rows of its own cone NaN.
"""
from __future__ import annotations

import math

import torch
from torch.autograd import forward_ad as fwAD

from cvxpylayers_amd.interfaces.cone_set import ConeSet, cone_rows, cones_key, normalize_cones

_SETS: dict = {}           # (cones key, device) -> ConeSet: one handle per cone set and device


def _cone_set(cones: dict, device: torch.device, cache: dict = _SETS) -> ConeSet:
    key = (cones_key(cones), str(device))
    if key not in cache:
        cache[key] = ConeSet(cones, device)
    return cache[key]


class _Project(torch.autograd.Function):

    @staticmethod
    def _f64(cset, t):
        return t.detach().to(torch.float64).reshape(-1, cset.m).contiguous()

    @staticmethod
    def forward(v, cset, dual, want_state):
        with torch.cuda.device(cset.device):
            out, state = cset.project(_Project._f64(cset, v), dual, want_state)
        return out.to(v.dtype).reshape(v.shape), state

    @staticmethod
    def setup_context(ctx, inputs, outputs):
        v, ctx.cset, ctx.dual, ctx.want_state = inputs
        ctx.state = outputs[1]
        if ctx.want_state:          # v itself is saved (rows and second-order cones re-derive their derivative from it): autograd checks that nobody overwrote it
            ctx.save_for_backward(v)
            ctx.save_for_forward(v)
        ctx.mark_non_differentiable(outputs[1]) if outputs[1] is not None else None

    @staticmethod
    def _dproject(ctx, g):
        (v,) = ctx.saved_tensors
        cset = ctx.cset
        with torch.cuda.device(cset.device):
            out = cset.dproject(_Project._f64(cset, v), ctx.state, _Project._f64(cset, g), ctx.dual)
        return out.to(v.dtype).reshape(v.shape)

    @staticmethod
    def jvp(ctx, tv, *_):
        if tv is None or not ctx.want_state:
            return None, None
        return _Project._dproject(ctx, tv), None

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _state):
        if g is None or not ctx.want_state:
            return None, None, None, None
        return _Project._dproject(ctx, g), None, None, None      # D Pi is symmetric: the same product


def _project(v, cones, dual, cache):
    cones = normalize_cones(cones)
    if not isinstance(v, torch.Tensor) or not v.is_floating_point():
        raise TypeError("project: v must be a floating-point tensor")
    m = cone_rows(cones)
    if v.dim() < 1 or v.shape[-1] != m or m == 0:
        raise ValueError(f"project: the last dimension of v is {v.shape[-1] if v.dim() else 'missing'}, the cones have {m} rows")
    if v.device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("cone projection needs a ROCm GPU; there is no CPU fallback")
    if v.numel() == 0:
        return v.clone()
    want_state = (torch.is_grad_enabled() and v.requires_grad) or fwAD.unpack_dual(v).tangent is not None
    out, _ = _Project.apply(v, _cone_set(cones, v.device, cache), bool(dual), want_state)
    return out


def project(v: torch.Tensor, cones: dict, dual: bool = False) -> torch.Tensor:
    """Pi_K(v) (dual=False) or Pi_K*(v) of v (..., m): leading dimensions are the batch, m the rows of `cones`.  ValueError when they disagree."""
    return _project(v, cones, dual, _SETS)


class ConeProjection(torch.nn.Module):
    """project(v, cones, dual) as a module: the cone set is fixed at construction, its handle is created once per device."""

    def __init__(self, cones: dict, dual: bool = False):
        super().__init__()
        self.cones = normalize_cones(cones)
        self.dual = bool(dual)
        self.rows = cone_rows(self.cones)
        self._sets: dict = {}

    def forward(self, v: torch.Tensor) -> torch.Tensor:
        return _project(v, self.cones, self.dual, self._sets)

    def extra_repr(self) -> str:
        return f"cones={self.cones}, dual={self.dual}"


def _svec_index(k: int, like: torch.Tensor, off_scale: float):
    # lower triangle (a >= b) in column-major order: the transposed row-major upper triangle; scale: 1 on the diagonal, off_scale elsewhere
    b, a = torch.triu_indices(k, k, device=like.device)
    scale = torch.full(a.shape, off_scale, dtype=like.dtype, device=like.device)
    scale[a == b] = 1.0
    return a, b, scale


def svec(X: torch.Tensor) -> torch.Tensor:
    """(..., k, k) symmetric -> (..., k (k + 1) / 2): lower triangle, column-major, off-diagonals scaled by sqrt(2)"""
    k = X.shape[-1]
    if X.dim() < 2 or X.shape[-2] != k:
        raise ValueError("svec: the last two dimensions must be square")
    a, b, scale = _svec_index(k, X, math.sqrt(2.0))
    return X[..., a, b] * scale


def smat(v: torch.Tensor, k: int) -> torch.Tensor:
    """the inverse of svec: (..., k (k + 1) / 2) -> (..., k, k) symmetric"""
    if v.shape[-1] != k * (k + 1) // 2:
        raise ValueError(f"smat: the last dimension must be {k * (k + 1) // 2} for order {k}")
    a, b, scale = _svec_index(k, v, math.sqrt(0.5))
    w = v * scale
    off = a != b
    X = v.new_zeros(v.shape[:-1] + (k * k,)).index_copy(-1, a * k + b, w).index_copy(-1, (b * k + a)[off], w[..., off])
    return X.reshape(v.shape[:-1] + (k, k))


def project_psd(X: torch.Tensor) -> torch.Tensor:
    """The projection of (X + X^T) / 2 onto the PSD cone, (..., k, k) -> (..., k, k) symmetric; differentiable with respect to X."""
    k = X.shape[-1]
    if X.dim() < 2 or X.shape[-2] != k:
        raise ValueError("project_psd: the last two dimensions must be square")
    return smat(project(svec(0.5 * (X + X.transpose(-1, -2))), {"s": [k]}), k)

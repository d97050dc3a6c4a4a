"""QuadEpigraph: a quadratic objective brought to cone form by differentiable torch ops."""
from __future__ import annotations

import numpy as np
import torch

from cvxpylayers_amd.interfaces.solver_args import SolverError


class QuadEpigraph:
    """min 1/2 x^T P x + q^T x + d  s.t.  A x + s = b, s in K      ==>      min t + q^T x + d  s.t. (same), and
           (t + 1, sqrt(2) L^T x, t - 1) in SOC(n + 2),   P = L L^T,
    because ||(sqrt(2) L^T x, t - 1)|| <= t + 1  <=>  1/2 x^T P x <= t.  This is the reduction CVXPY itself applies when a solver has
    no quadratic objective (what DIFFCP receives); doing it here, on device tensors under autograd, lets P be a *parameter*: the
    Cholesky factor is computed per instance (batched, differentiable), its entries become entries of A_eval, and the gradient
    with respect to P flows back through torch's Cholesky derivative.  One extra variable (t, last) and one extra SOC block,
    placed after the template's own SOC blocks (SCS row order z, l, q, s, ep, p); the template's rows keep their relative order.

    P_eval holds the values of P in the CSC structure `objective_structure = (indices, indptr, (n, n))`; a structure with all
    entries on or above (or on or below) the diagonal is read as one triangle of the symmetric matrix."""

    def __init__(self, objective_structure, A_structure, A_shape, cone_dict):
        p_indices, p_indptr, (n, n2) = objective_structure
        m, np1 = A_shape
        assert n == n2 == np1 - 1, "P must be n x n"
        self.n, self.m = int(n), int(m)
        self.p_rows = np.asarray(p_indices, dtype=np.int64)
        self.p_cols = np.repeat(np.arange(n), np.diff(np.asarray(p_indptr))).astype(np.int64)
        self.one_triangle = bool(len(self.p_rows)) and (bool((self.p_rows <= self.p_cols).all()) or bool((self.p_rows >= self.p_cols).all()))
        self.p_indices, self.p_indptr = np.asarray(p_indices, dtype=np.int32), np.asarray(p_indptr, dtype=np.int32)
        # native (in-kernel) P needs symmetric values: for a full structure, entry (i, j) is averaged with entry (j, i); sym_perm
        # is that pairing (identity for one-triangle structures, None when the structure is not symmetric -> epigraph form only)
        if self.one_triangle or len(self.p_rows) == 0:
            self.sym_perm = np.arange(len(self.p_rows))
        else:
            pos = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(self.p_rows, self.p_cols))}
            perm = [pos.get((int(c), int(r)), -1) for r, c in zip(self.p_rows, self.p_cols)]
            self.sym_perm = np.asarray(perm) if min(perm) >= 0 else None
        a_idx, a_ptr = np.asarray(A_structure[0], dtype=np.int64), np.asarray(A_structure[1], dtype=np.int64)
        nnz_old = int(a_ptr[-1])
        r0 = int(cone_dict.get("z", 0)) + int(cone_dict.get("l", 0)) + int(sum(cone_dict.get("q", [])))      # first row of the new SOC block
        self.r0 = r0
        d = n + 2
        self.m_aug = m + d
        remap = np.where(np.arange(m) < r0, np.arange(m), np.arange(m) + d)       # template row -> augmented row
        self.dual_rows = remap
        # entries of the augmented [A_cvx | b_cvx] (columns x_0..x_{n-1}, t, b), sorted by (column, row); source index into
        # cat([A_eval (nnz_old), sqrt(2) * L[j, k] for the n(n+1)/2 pairs j >= k, +1, -1]) per instance
        tri_j, tri_k = np.tril_indices(n)
        self.tri_j, self.tri_k = tri_j, tri_k
        ntri = len(tri_j)
        ONE, MINUS = nnz_old + ntri, nnz_old + ntri + 1
        a_cols = np.repeat(np.arange(np1), np.diff(a_ptr))
        ent = []          # (col, row, source)
        for kk in range(nnz_old):
            c_ = int(a_cols[kk])
            ent.append((c_ if c_ < n else n + 1, int(remap[a_idx[kk]]), kk))
        for e in range(ntri):          # A_cvx[r0 + 1 + k, j] = sqrt(2) L[j, k]
            ent.append((int(tri_j[e]), r0 + 1 + int(tri_k[e]), nnz_old + e))
        ent.append((n, r0, ONE)); ent.append((n, r0 + n + 1, ONE))               # t in the first and the last row of the block
        ent.append((n + 1, r0, ONE)); ent.append((n + 1, r0 + n + 1, MINUS))     # b = (1, 0, ..., 0, -1)
        ent.sort()
        self.aug_indices = np.asarray([e[1] for e in ent], dtype=np.int32)
        counts = np.bincount(np.asarray([e[0] for e in ent]), minlength=n + 2)
        self.aug_indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.src = np.asarray([e[2] for e in ent], dtype=np.int64)
        self.aug_cones = {**cone_dict, "q": list(cone_dict.get("q", [])) + [d]}
        self._dev = {}

    def _idx(self, device):
        key = str(device)
        if key not in self._dev:
            t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).to(device)
            self._dev[key] = dict(src=t(self.src), pr=t(self.p_rows), pc=t(self.p_cols), tj=t(self.tri_j), tk=t(self.tri_k), dual=t(self.dual_rows))
        return self._dev[key]

    def assemble(self, P_eval, q_eval, A_eval):
        """(nnz_P, B), (n+1, B), (nnz_aug, B)  ->  q_aug (n+2, B), A_aug (nnz_aug', B); differentiable torch ops"""
        ix = self._idx(A_eval.device)
        n, B = self.n, A_eval.shape[1]
        f64 = dict(dtype=torch.float64, device=A_eval.device)
        Pd = torch.zeros((B, n * n), **f64).index_add(1, ix["pr"] * n + ix["pc"], P_eval.to(torch.float64).t()).reshape(B, n, n)
        if self.one_triangle:
            Pd = Pd + Pd.transpose(1, 2) - torch.diag_embed(torch.diagonal(Pd, dim1=1, dim2=2))
        else:
            Pd = 0.5 * (Pd + Pd.transpose(1, 2))
        # P is positive semidefinite, possibly singular: a relative jitter keeps the factorisation defined (1e-12 of the largest
        # diagonal entry: far below the solver tolerance)
        jit = 1e-12 * torch.diagonal(Pd, dim1=1, dim2=2).abs().amax(dim=1).clamp_min(1e-300) + 1e-300
        Lf, info = torch.linalg.cholesky_ex(Pd + jit[:, None, None] * torch.eye(n, **f64))
        if bool((info != 0).any()):
            raise SolverError("MI355 solver: the quadratic objective matrix P is not positive semidefinite "
                              f"(Cholesky failed for {int((info != 0).sum())} of {B} instances)")
        Lvals = (2.0 ** 0.5) * Lf[:, ix["tj"], ix["tk"]].t()                      # (n(n+1)/2, B)
        one = torch.ones((1, B), **f64)
        source = torch.cat([A_eval.to(torch.float64), Lvals, one, -one], dim=0)
        A_aug = source.index_select(0, ix["src"])
        q64 = q_eval.to(torch.float64)
        q_aug = torch.cat([q64[:n], one, q64[n:n + 1]], dim=0)
        return q_aug, A_aug

    def split(self, primal_aug, dual_aug):
        ix = self._idx(dual_aug.device)
        return primal_aug[:, :self.n], dual_aug.index_select(1, ix["dual"])

"""Parameter gradients straight from the adjoint's factors (solver_args param_grad="factors"): the transposed parameter maps of a layer, composed once into the one
packed CSR that k_param_grad reads (csrc/ce_param_grad.h, include/cone_engine.h ce_vjp_many_params / ce_vjp_params), and its device copies."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch

Q_FLAG = np.int32(-2 ** 31)          # a code with the sign bit set addresses dq


P_FLAG = np.int32(1 << 30)           # with the sign bit: an entry of dP (a dq code has bit 30 clear: n < 2^15)


def compose_maps(A_mapT, q_mapT, indices, indptr, n: int, m: int, P_mapT=None, prow=None, pcol=None, p_tri: bool = False, sym_perm=None):
    """(ptr, code, kidx, val) of the composed map: CSR over the rows of the transposed maps (the parameter columns 0 .. Ptot, the constant column included).
    A_mapT (rows, nnz_aug), q_mapT (rows, n + 1): the transposed parameter maps; indices / indptr: the CSC structure of [A | b] (m x (n + 1)), whose value
    order the columns of A_mapT follow.  Per row the A entries come first (in value order), the q entries behind them (in dq order).
    code >= 0: the entry's (row i, column j) packed as i | j << 16 (j == n: the b column), kidx its position in the value order;
    code <  0: entry (code & 0x7fffffff) of dq, kidx 0.
    P_mapT (rows, nnz_p), optional (a native QP: ce_vjp_qp_many_params): the transposed P map, its columns in the order of P's structure prow / pcol (entry k is
    (prow[k], pcol[k])).  Its entries stand per row behind the q entries (in structure order): code = sign bit | bit 30 | i | j << 15, kidx = k.  The kernel
    evaluates ONE share -1/2 (r_x,i x_j + r_x,j x_i) per entry; what the dA route does to dP besides is exact or linear and goes into val here:
      p_tri (a one-triangle structure): an entry with i != j stands for both matrix entries, val is doubled (exact);
      sym_perm (a full structure whose values the frontend symmetrises, P <- (P + P[sym_perm]) / 2): the transpose, val / 2 on entry k and val / 2 on entry
      sym_perm[k] -- the two fall together on the diagonal, and with another map entry of the row that addresses the same k.
    Without P_mapT the output is what it was without these arguments."""
    A_mapT, q_mapT = sp.csr_array(A_mapT).astype(np.float64), sp.csr_array(q_mapT).astype(np.float64)
    A_mapT.sort_indices(); q_mapT.sort_indices()
    rows = int(A_mapT.shape[0])
    indices, indptr = np.asarray(indices, dtype=np.int64), np.asarray(indptr, dtype=np.int64)
    nnz_aug = int(indptr[-1])
    if q_mapT.shape[0] != rows or A_mapT.shape[1] != nnz_aug or q_mapT.shape[1] != n + 1 or indptr.size != n + 2:
        raise ValueError(f"compose_maps: maps of shapes {A_mapT.shape}, {q_mapT.shape} do not belong to a structure with n = {n}, nnz_aug = {nnz_aug}")
    if m >= (1 << 16) or n >= (1 << 15):
        raise ValueError(f"compose_maps: the packed (row, column) of an entry needs m < 65536 and n < 32768, got m = {m}, n = {n}")
    colidx = np.repeat(np.arange(n + 1, dtype=np.int64), np.diff(indptr))
    if indices.size and (indices.min() < 0 or indices.max() >= m):
        raise ValueError("compose_maps: a row index of the structure is out of range")
    cntA, cntq = np.diff(A_mapT.indptr), np.diff(q_mapT.indptr)
    cntP = np.zeros(rows, dtype=cntA.dtype)
    if P_mapT is not None:
        if prow is None or pcol is None:
            raise ValueError("compose_maps: a P map needs P's structure (prow, pcol)")
        prow, pcol = np.asarray(prow, dtype=np.int64), np.asarray(pcol, dtype=np.int64)
        P_mapT = sp.coo_array(P_mapT).astype(np.float64)
        if P_mapT.shape != (rows, prow.size) or pcol.size != prow.size:
            raise ValueError(f"compose_maps: a P map of shape {P_mapT.shape} does not belong to {rows} rows and a structure of {prow.size} entries")
        if prow.size and (min(prow.min(), pcol.min()) < 0 or max(prow.max(), pcol.max()) >= n):
            raise ValueError("compose_maps: an index of P's structure is out of range")
        pr, pc, pv = P_mapT.row, P_mapT.col, P_mapT.data
        if sym_perm is not None:
            sym_perm = np.asarray(sym_perm, dtype=np.int64)
            if sym_perm.shape != prow.shape:
                raise ValueError("compose_maps: sym_perm does not belong to P's structure")
            pr, pc, pv = np.concatenate([pr, pr]), np.concatenate([pc, sym_perm[pc]]), np.concatenate([0.5 * pv, 0.5 * pv])
        P_mapT = sp.csr_array((pv, (pr, pc)), shape=(rows, prow.size))          # (duplicates are summed)
        P_mapT.sort_indices()
        cntP = np.diff(P_mapT.indptr)
    ptr = np.concatenate([[0], np.cumsum(cntA + cntq + cntP)]).astype(np.int64)
    if ptr[-1] >= 2 ** 31:
        raise ValueError("compose_maps: more than 2^31 - 1 map entries")
    tot = int(ptr[-1])
    code, kidx, val = np.zeros(tot, dtype=np.int32), np.zeros(tot, dtype=np.int32), np.zeros(tot, dtype=np.float64)
    # positions of the A entries: row r's run starts at ptr[r]; of the q entries: at ptr[r] + cntA[r]; of the P entries: at ptr[r] + cntA[r] + cntq[r]
    rowA = np.repeat(np.arange(rows), cntA)
    posA = ptr[rowA] + (np.arange(A_mapT.nnz) - A_mapT.indptr[rowA])
    k = A_mapT.indices.astype(np.int64)
    code[posA] = (indices[k] | (colidx[k] << 16)).astype(np.int32)
    kidx[posA] = k.astype(np.int32)
    val[posA] = A_mapT.data
    rowq = np.repeat(np.arange(rows), cntq)
    posq = ptr[rowq] + cntA[rowq] + (np.arange(q_mapT.nnz) - q_mapT.indptr[rowq])
    code[posq] = q_mapT.indices.astype(np.int32) | Q_FLAG
    val[posq] = q_mapT.data
    if P_mapT is not None:
        rowP = np.repeat(np.arange(rows), cntP)
        posP = ptr[rowP] + cntA[rowP] + cntq[rowP] + (np.arange(P_mapT.nnz) - P_mapT.indptr[rowP])
        k = P_mapT.indices.astype(np.int64)
        code[posP] = (prow[k] | (pcol[k] << 15)).astype(np.int32) | P_FLAG | Q_FLAG
        kidx[posP] = k.astype(np.int32)
        val[posP] = np.where(bool(p_tri) & (prow[k] != pcol[k]), 2.0 * P_mapT.data, P_mapT.data)
    return ptr.astype(np.int32), code, kidx, val


class ComposedMaps:
    """The composed map of one layer and its device copies (lazily per device): what ConeEngine.vjp_many_params / vjp_params take as `maps`."""

    def __init__(self, A_mapT, q_mapT, indices, indptr, n: int, m: int, P_mapT=None, prow=None, pcol=None, p_tri: bool = False, sym_perm=None):
        self.ptr, self.code, self.kidx, self.val = compose_maps(A_mapT, q_mapT, indices, indptr, n, m, P_mapT, prow, pcol, p_tri, sym_perm)
        self.rows = int(self.ptr.size) - 1
        self.n, self.m, self.nnz_aug = int(n), int(m), int(np.asarray(indptr)[-1])
        self.nnz_p = 0 if P_mapT is None else int(np.asarray(prow).size)
        self._dev: dict = {}

    def on(self, device: torch.device):
        key = (device.type, device.index)
        if key not in self._dev:
            pad = lambda a: a if a.size else np.zeros(1, dtype=a.dtype)          # (an empty map still hands the library non-null pointers)
            self._dev[key] = tuple(torch.from_numpy(pad(a)).to(device) for a in (self.ptr, self.code, self.kidx, self.val))
        return self._dev[key]

"""Parameter gradients straight from the adjoint's factors (solver_args param_grad="factors"): the transposed parameter maps of a layer, composed once into the one
packed CSR that k_param_grad reads (csrc/ce_param_grad.h, include/cone_engine.h ce_vjp_many_params / ce_vjp_params), and its device copies."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch

Q_FLAG = np.int32(-2 ** 31)          # a code with the sign bit set addresses dq


def compose_maps(A_mapT, q_mapT, indices, indptr, n: int, m: int):
    """(ptr, code, kidx, val) of the composed map: CSR over the rows of the transposed maps (the parameter columns 0 .. Ptot, the constant column included).
    A_mapT (rows, nnz_aug), q_mapT (rows, n + 1): the transposed parameter maps; indices / indptr: the CSC structure of [A | b] (m x (n + 1)), whose value
    order the columns of A_mapT follow.  Per row the A entries come first (in value order), the q entries behind them (in dq order).
    code >= 0: the entry's (row i, column j) packed as i | j << 16 (j == n: the b column), kidx its position in the value order;
    code <  0: entry (code & 0x7fffffff) of dq, kidx 0."""
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
    ptr = np.concatenate([[0], np.cumsum(cntA + cntq)]).astype(np.int64)
    if ptr[-1] >= 2 ** 31:
        raise ValueError("compose_maps: more than 2^31 - 1 map entries")
    tot = int(ptr[-1])
    code, kidx, val = np.zeros(tot, dtype=np.int32), np.zeros(tot, dtype=np.int32), np.zeros(tot, dtype=np.float64)
    # positions of the A entries: row r's run starts at ptr[r]; of the q entries: at ptr[r] + cntA[r]
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
    return ptr.astype(np.int32), code, kidx, val


class ComposedMaps:
    """The composed map of one layer and its device copies (lazily per device): what ConeEngine.vjp_many_params / vjp_params take as `maps`."""

    def __init__(self, A_mapT, q_mapT, indices, indptr, n: int, m: int):
        self.ptr, self.code, self.kidx, self.val = compose_maps(A_mapT, q_mapT, indices, indptr, n, m)
        self.rows = int(self.ptr.size) - 1
        self.n, self.m, self.nnz_aug = int(n), int(m), int(np.asarray(indptr)[-1])
        self._dev: dict = {}

    def on(self, device: torch.device):
        key = (device.type, device.index)
        if key not in self._dev:
            pad = lambda a: a if a.size else np.zeros(1, dtype=a.dtype)          # (an empty map still hands the library non-null pointers)
            self._dev[key] = tuple(torch.from_numpy(pad(a)).to(device) for a in (self.ptr, self.code, self.kidx, self.val))
        return self._dev[key]

"""ConeSet: one ce_cones_handle (one product of cones, one device) behind ce_cone_project / ce_cone_dproject of include/cone_engine.h."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd.problems import cone_rows  # noqa: F401  (re-exported)


def normalize_cones(cones) -> dict:
    """The cone dict with every key present and plain python values, validated on the host: {"z", "l", "q": [...], "s": [...], "ep", "p": [...]}."""
    if not isinstance(cones, dict):
        raise TypeError(f"cones must be a dict with keys z, l, q, s, ep, p; got {type(cones).__name__}")
    unknown = set(cones) - {"z", "f", "l", "q", "s", "ep", "p"}
    if unknown:
        raise ValueError(f"unknown cone keys {sorted(unknown)}")
    out = {"z": int(cones.get("z", cones.get("f", 0))), "l": int(cones.get("l", 0)), "q": [int(d) for d in cones.get("q", [])],
           "s": [int(k) for k in cones.get("s", [])], "ep": int(cones.get("ep", 0)), "p": [float(a) for a in cones.get("p", [])]}
    if out["z"] < 0 or out["l"] < 0 or out["ep"] < 0:
        raise ValueError("cone counts must be non-negative")
    if any(d < 1 for d in out["q"]):
        raise ValueError("second-order cone dimensions must be at least 1")
    if any(k < 1 for k in out["s"]):
        raise ValueError("PSD orders must be at least 1")
    if any(not (0.0 < abs(a) < 1.0) for a in out["p"]):
        raise ValueError("power cone exponents must lie in (0, 1) (or (-1, 0) for the dual cone)")
    return out


def cones_key(cones: dict) -> tuple:
    return (cones["z"], cones["l"], tuple(cones["q"]), tuple(cones["s"]), cones["ep"], tuple(cones["p"]))


class ConeSet:
    """Owns one ce_cones_handle.  project / dproject take (B, m) float64 tensors on the set's device whose rows are contiguous (any row pitch >= m) and launch
    on the current stream."""

    def __init__(self, cones: dict, device: torch.device):
        self._h = None
        L = _lib.lib()
        self.device = device
        self.cones = normalize_cones(cones)
        q = np.ascontiguousarray(self.cones["q"], dtype=np.int32)
        s = np.ascontiguousarray(self.cones["s"], dtype=np.int32)
        p = np.ascontiguousarray(self.cones["p"], dtype=np.float64)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        h = C.c_void_p()
        rc = L.ce_cones_create(self.cones["z"], self.cones["l"], len(q), q.ctypes.data_as(ip), len(s), s.ctypes.data_as(ip), self.cones["ep"], len(p),
                               p.ctypes.data_as(dp), device.index or 0, C.byref(h))
        if rc == -3:          # CE_E_TOO_LARGE: a PSD order beyond the LDS-resident kernels
            raise NotImplementedError(L.ce_last_error().decode())
        _lib.check(rc, "ce_cones_create")
        self._h = h
        self.m = int(L.ce_cones_rows(h))
        self.state_len = int(L.ce_cones_state_len(h))
        self.project_calls = 0            # introspection (tests): calls of project, and how many of them asked for the derivative state
        self.state_calls = 0

    def __del__(self):
        try:
            if self._h:
                _lib.lib().ce_cones_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, t: torch.Tensor, what: str):
        if t.dtype != torch.float64 or t.device != self.device or t.dim() != 2 or t.shape[1] != self.m or (t.shape[1] > 1 and t.stride(1) != 1) or \
                (t.shape[0] > 1 and t.stride(0) < self.m):
            raise ValueError(f"ConeSet: {what} must be (B, {self.m}) float64 on {self.device} with contiguous rows")

    @staticmethod
    def _pitch(t: torch.Tensor) -> int:
        return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])

    def project(self, v: torch.Tensor, dual: bool = False, want_state: bool = False):
        """(Pi(v), state): state (B, state_len) for dproject, or None when not wanted (nothing of the derivative is then computed)"""
        self._check(v, "v")
        B = v.shape[0]
        with torch.cuda.device(self.device):
            out = torch.empty((B, self.m), device=self.device, dtype=torch.float64)
            state = torch.empty((B, self.state_len), device=self.device, dtype=torch.float64) if want_state else None
            self.project_calls += 1
            self.state_calls += int(want_state)
            _lib.check(_lib.lib().ce_cone_project(self._h, B, v.data_ptr(), self._pitch(v), int(bool(dual)), out.data_ptr(), self.m,
                                                  state.data_ptr() if (want_state and self.state_len) else None, self._stream()), "ce_cone_project")
        return out, state

    def dproject(self, v: torch.Tensor, state: torch.Tensor, direction: torch.Tensor, dual: bool = False) -> torch.Tensor:
        """D Pi(v) direction, with the state the matching project(v, dual, want_state=True) returned"""
        self._check(v, "v")
        self._check(direction, "direction")
        B = v.shape[0]
        if direction.shape[0] != B or state is None or state.shape != (B, self.state_len):
            raise ValueError("ConeSet.dproject: direction and state must belong to the same batch as v")
        with torch.cuda.device(self.device):
            out = torch.empty((B, self.m), device=self.device, dtype=torch.float64)
            _lib.check(_lib.lib().ce_cone_dproject(self._h, B, v.data_ptr(), self._pitch(v), int(bool(dual)), state.data_ptr() if self.state_len else None,
                                                   direction.data_ptr(), self._pitch(direction), out.data_ptr(), self.m, self._stream()), "ce_cone_dproject")
        return out

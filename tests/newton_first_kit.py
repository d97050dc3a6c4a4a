"""Shared by test_gpu_check_solved.py and test_gpu_newton_first.py: the numpy float64 statement of the forward kernels' termination test (include/cone_engine.h
ce_check_solved; ce_forward_v2.h and oracle/cone_oracle.c at tau = 1), the perturbation recipe the feature was specified with, and the shapes.  Nothing here
needs a GPU.

    res_pri  = |A x + s - b|_inf        prl = max(|A x|_inf, |s|_inf, |b|_inf)
    res_dual = |P x + A^T y + c|_inf    drl = max(|A^T y|_inf, |c|_inf, |P x|_inf)
    gap      = |x^T P x + c^T x + b^T y|      grl = max(|c^T x|, |b^T y|, |x^T P x|)
    solved  <=>  eligible, all finite, and each of the three <= eps_abs + eps_rel * its scale
"""
from __future__ import annotations

import numpy as np

from cvxpylayers_amd import problems as P

SMALL = (12, {"z": 2, "l": 8, "q": [4, 5]}, 64, 1)                                      # n, cones, B, seed
METRIC = (P.CONFIGS["M"]["n"], P.CONFIGS["M"]["cones"], 48, 0)


def perturb(A, b, c, rel, seed):
    """every entry of A, b, c multiplied by 1 + rel N(0, 1), drawn in that order from default_rng(seed + 100)"""
    rng = np.random.default_rng(seed + 100)
    return tuple(t * (1.0 + rel * rng.standard_normal(t.shape)) for t in (A, b, c))


def termination_test(A, b, c, x, y, s, eps_abs, eps_rel, Pm=None, eligible=None):
    """A (B, m, n), b (B, m), c (B, n), the point x (B, n), y, s (B, m), Pm (B, n, n) symmetric or None.  Returns a dict: solved (B,) bool, resid (B, 3), thr (B, 3)
    the three thresholds, passed (B, 3) bool, finite (B,) bool, and terms (B, 3): the sum of |terms| of the row (of the whole sum, for the gap) that attains
    each residual -- the scale of its rounding error."""
    B, m, n = A.shape
    with np.errstate(all="ignore"):
        Ax = np.einsum("bij,bj->bi", A, x); ATy = np.einsum("bij,bi->bj", A, y)
        Px = np.einsum("bij,bj->bi", Pm, x) if Pm is not None else np.zeros((B, n))
        rp, rd = np.abs(Ax + s - b), np.abs(Px + ATy + c)
        ctx, bty, xPx = (c * x).sum(1), (b * y).sum(1), (x * Px).sum(1)
        resid = np.stack([rp.max(1), rd.max(1), np.abs(xPx + ctx + bty)], axis=1)
        prl = np.maximum(np.maximum(np.abs(Ax).max(1), np.abs(s).max(1)), np.abs(b).max(1))
        drl = np.maximum(np.maximum(np.abs(ATy).max(1), np.abs(c).max(1)), np.abs(Px).max(1))
        grl = np.maximum(np.maximum(np.abs(ctx), np.abs(bty)), np.abs(xPx))
        thr = eps_abs + eps_rel * np.stack([prl, drl, grl], axis=1)
        finite = np.isfinite(x).all(1) & np.isfinite(y).all(1) & np.isfinite(s).all(1) & np.isfinite(resid).all(1) & np.isfinite(thr).all(1)
        passed = resid <= thr
        rows_p = (np.abs(A) * np.abs(x)[:, None, :]).sum(2) + np.abs(s) + np.abs(b)
        rows_d = (np.abs(A) * np.abs(y)[:, :, None]).sum(1) + np.abs(c)
        quad = np.zeros(B)
        if Pm is not None:
            rows_d = rows_d + (np.abs(Pm) * np.abs(x)[:, None, :]).sum(2)
            quad = (np.abs(Pm) * np.abs(x)[:, None, :] * np.abs(x)[:, :, None]).sum((1, 2))
        ar = np.arange(B)
        terms = np.stack([rows_p[ar, np.nan_to_num(rp, nan=0.0).argmax(1)], rows_d[ar, np.nan_to_num(rd, nan=0.0).argmax(1)],
                          quad + np.abs(c * x).sum(1) + np.abs(b * y).sum(1)], axis=1)
    solved = finite & passed.all(1)
    if eligible is not None:
        solved = solved & np.asarray(eligible, bool)
    return dict(solved=solved, resid=resid, thr=thr, passed=passed, finite=finite, terms=terms)


def margins(t):
    """|resid - thr| / thr of the finite instances of a termination_test result: how far every comparison is from flipping"""
    f = t["finite"]
    return (np.abs(t["resid"][f] - t["thr"][f]) / t["thr"][f])

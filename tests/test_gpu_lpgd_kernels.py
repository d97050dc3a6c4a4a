"""The two streaming kernels of the LPGD backward alone, through the C ABI (ce_lpgd_perturb, ce_lpgd_grad; csrc/ce_lpgd.h) against numpy in np.longdouble.
The formulas hold at any values, so the data is random: no program is solved here.  Bounds (derived, not measured):
  * ce_lpgd_perturb: q_out = fma(-rho, x, fma(tau, dx, q)) rounds once per fma, half an ulp of that fma's result: within 1 ulp of the largest of
    |q|, |tau dx|, |rho x| and the two results; a b slot fma(-tau, dy, b) rounds once: within 1 ulp of max(|b|, |tau dy|).  Every other slot of the A copy and
    every off-diagonal entry of P_out is bit-equal to its input; a diagonal entry of P_out is the one rounded sum P + rho: bit-equal to numpy's.
  * ce_lpgd_grad: the staged form  -(y_b,r Dx_c + Dy_r x_a,c) / delta  with Dx, Dy rounded once, divided once, multiplied and added once each: at most
    5 roundings of relative size 2^-53 on either term -- within 8 * 2^-53 (|y_b,r Dx_c| + |Dy_r x_a,c|) / delta as the issue sets it; the same for dq and dP.
Every case fails on a library without the two entry points."""
import numpy as np
import pytest
import torch

import lpgd_kit as lk
import value_kit as vk
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LD = np.longdouble
U = 2.0 ** -53
SENTINEL = 777.25
GUARD = 37


def _engine(tpl, struct=None):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    return ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, DEV, p_structure=struct[:2] if struct is not None else None)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(size, dtype=torch.float64):
    buf = torch.full((2 * GUARD + max(size, 1),), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + size]


def _guards_intact(buf, size):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + max(size, 1):] == SENTINEL).all())


def _struct_dev(struct):
    pr, pc, _ = vk.p_entries(struct)
    return _cuda(pr.astype(np.int32)), _cuda(pc.astype(np.int32))


def _template(name):
    n, cones, B, seed, sparse = vk.KERNEL_SHAPES[name]
    if sparse:
        pattern, b_pattern = vk.sparse_patterns(n, cones, seed)
        return P.dense_template(n, cones, pattern=pattern, b_pattern=b_pattern), B
    return P.dense_template(n, cones), B


def _bpos(tpl):
    """position of every row's b entry in the value order, -1 where the template has none"""
    n = tpl.n
    bpos = np.full(tpl.m, -1)
    bpos[np.asarray(tpl.indices)[tpl.indptr[n]:tpl.indptr[n + 1]]] = np.arange(tpl.indptr[n], tpl.indptr[n + 1])
    return bpos


# ------------------------------------------------------------------------------------------------ ce_lpgd_perturb
def _raw_perturb(eng, A_bm, q, q_layout, x, dx, dy, tau, rho, P_vals=None, struct=None):
    """ce_lpgd_perturb into guarded, sentinel-filled buffers.  Returns numpy q_out (n+1, B), A_out (B, K), P_out (B, nnz_p) and flags (B,); an output the call
    must not touch comes back as None after its buffer was found full of sentinels."""
    B, K, n = x.shape[0], eng.nnz_aug, eng.n
    nnz_p = len(struct[0]) if struct is not None else 0
    q_t = _cuda(q) if q_layout == "minor" else _cuda(q.T).t()          # (n+1, B): contiguous, or a view of batch-major storage
    bq, vq = _guarded((n + 1) * B); bA, vA = _guarded(K * B); bP, vP = _guarded(nnz_p * B)
    bf, vf = _guarded(B, torch.int32)
    bf[:] = 777; SENT_I = 777
    A_t = _cuda(A_bm)
    pst = _struct_dev(struct) if struct is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    xt, dxt, dyt, Pt = _cuda(x), _cuda(dx), (_cuda(dy) if dy is not None else None), (_cuda(P_vals) if P_vals is not None else None)
    rc = _lib.lib().ce_lpgd_perturb(eng._h, B, A_t.data_ptr(), K, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), ptr(Pt), pst[0].data_ptr() if pst else None,
                                    pst[1].data_ptr() if pst else None, nnz_p, xt.data_ptr(), dxt.data_ptr(), ptr(dyt), float(tau), float(rho),
                                    vq.data_ptr(), vA.data_ptr(), vP.data_ptr() if nnz_p else None, vf.data_ptr(), eng._stream())
    _lib.check(rc, "ce_lpgd_perturb")
    torch.cuda.synchronize()
    assert _guards_intact(bq, (n + 1) * B) and _guards_intact(bA, K * B) and _guards_intact(bP, nnz_p * B), "a guard band was written"
    assert (bf[:GUARD] == SENT_I).all() and (bf[GUARD + B:] == SENT_I).all()
    q_out = (vq.view(n + 1, B) if q_layout == "minor" else vq.view(B, n + 1).t()).cpu().numpy()
    A_out = vA.view(B, K).cpu().numpy() if dy is not None else None
    if dy is None:
        assert (bA == SENTINEL).all(), "dy = NULL: the A output was touched"
    P_out = vP.view(B, nnz_p).cpu().numpy() if (nnz_p and rho != 0.0) else None
    if nnz_p and rho == 0.0:
        assert (bP == SENTINEL).all(), "rho = 0: the P output was touched"
    return q_out, A_out, P_out, vf.cpu().numpy()


def _check_perturb(tpl, B, q_layout, with_dy, tau, rho, seed):
    eng = _engine(tpl)
    n, m, K = tpl.n, tpl.m, tpl.nnz_aug
    rng = np.random.default_rng(seed)
    A_bm, q = rng.standard_normal((B, K)), rng.standard_normal((n + 1, B))
    x, dx, dy = rng.standard_normal((B, n)), rng.standard_normal((B, n)), rng.standard_normal((B, m))
    bpos = _bpos(tpl)
    no_slot = np.nonzero(bpos < 0)[0]
    # instances built to set each flag: 0 has an all-zero cotangent; 1 (when the batch has one) a zero dx and a dy that is zero except -- where the template has
    # such a row -- on a row without a b slot; on that row every OTHER instance has dy = 0, so only instance 1 sets bit 1
    dx[0] = 0.0; dy[0] = 0.0
    if len(no_slot):
        dy[:, no_slot] = 0.0
    if B > 1:
        dx[1] = 0.0; dy[1] = 0.0
        if len(no_slot):
            dy[1, no_slot[0]] = 0.5
        else:
            dy[1, 0] = 0.5
    q_out, A_out, _, flags = _raw_perturb(eng, A_bm, q, q_layout, x, dx, dy if with_dy else None, tau, rho)
    # q
    t1 = q[:n].astype(LD) + LD(tau) * dx.T.astype(LD)
    res = t1 - LD(rho) * x.T.astype(LD)
    big = np.maximum.reduce([np.abs(q[:n]), np.abs(tau * dx.T), np.abs(rho * x.T), np.abs(t1).astype(float), np.abs(res).astype(float)])
    err = np.abs(q_out[:n].astype(LD) - res).astype(float)
    print(f"q_out: max error {float((err / np.spacing(big)).max()):.2f} ulp of the largest term")
    assert (err <= np.spacing(big)).all()
    assert np.array_equal(q_out[n], q[n]), "the constant row of q must be copied"
    # flags
    want = np.zeros(B, dtype=int)
    zero = (dx == 0).all(axis=1) & ((dy == 0).all(axis=1) if with_dy else True)
    want[zero] |= 1
    if with_dy and len(no_slot):
        want[(dy[:, no_slot] != 0).any(axis=1)] |= 2
    assert np.array_equal(flags, want), (flags, want)
    assert flags[0] == 1 and (B == 1 or not with_dy or flags[1] == (2 if len(no_slot) else 0))
    # A
    if with_dy:
        slots = bpos[bpos >= 0]
        others = np.setdiff1d(np.arange(K), slots)
        assert np.array_equal(A_out[:, others].view(np.int64), A_bm[:, others].view(np.int64)), "a slot that is no b entry changed"
        rows = np.nonzero(bpos >= 0)[0]
        exact = A_bm[:, slots].astype(LD) - LD(tau) * dy[:, rows].astype(LD)
        big = np.maximum(np.abs(A_bm[:, slots]), np.abs(tau * dy[:, rows]))
        err = np.abs(A_out[:, slots].astype(LD) - exact).astype(float)
        assert (err <= np.spacing(big)).all()
        assert len(slots) and (B <= 2 or np.abs(A_out[:, slots] - A_bm[:, slots]).max() > 1e-3)          # (instances 0 and 1 carry the flag constructions)
    else:
        assert A_out is None


@pytest.mark.parametrize("q_layout", ["minor", "major"])
@pytest.mark.parametrize("with_dy", [True, False])
@pytest.mark.parametrize("name", ["tiny_b1", "dense_b5", "sparse_b5", "sparse_b65"])
def test_perturb_equals_numpy(name, with_dy, q_layout):
    tpl, B = _template(name)
    _check_perturb(tpl, B, q_layout, with_dy, tau=0.37, rho=0.0, seed=3)
    _check_perturb(tpl, B, q_layout, with_dy, tau=-0.021, rho=0.8, seed=4)          # (the -tau side, with the proximal term)


@pytest.mark.parametrize("kind", ["full", "one_triangle"])
def test_perturb_adds_rho_on_the_diagonal_of_P(kind):
    from qp_ns_kit import full_structure
    from test_quad_objective import _upper_structure
    n, cones, B, seed = vk.QP_SHAPE
    struct = full_structure(n) if kind == "full" else _upper_structure(n)
    tpl = P.dense_template(n, cones)
    eng = _engine(tpl)
    rng = np.random.default_rng(seed)
    pr, pc, _ = vk.p_entries(struct)
    P_vals = rng.standard_normal((B, len(pr)))
    A_bm, q = rng.standard_normal((B, tpl.nnz_aug)), rng.standard_normal((n + 1, B))
    x, dx = rng.standard_normal((B, n)), rng.standard_normal((B, n))
    _, _, P_out, _ = _raw_perturb(eng, A_bm, q, "minor", x, dx, None, 0.1, 0.7, P_vals=P_vals, struct=struct)
    want = P_vals + np.where(pr == pc, 0.7, 0.0)[None]
    assert (pr == pc).sum() == n and np.array_equal(P_out.view(np.int64), want.view(np.int64))
    _raw_perturb(eng, A_bm, q, "minor", x, dx, None, 0.1, 0.0, P_vals=P_vals, struct=struct)          # rho = 0: P_out untouched (checked inside)


# ------------------------------------------------------------------------------------------------ ce_lpgd_grad
def _raw_grad(eng, xa, ya, xb, yb, delta, skip=None, A_layout="major", q_layout="minor", struct=None):
    """ce_lpgd_grad into guarded buffers: numpy dA (nnz_aug, B), dq (n+1, B), dP (B, nnz_p) or None"""
    B, K, n = xa.shape[0], eng.nnz_aug, eng.n
    nnz_p = len(struct[0]) if struct is not None else 0
    bA, vA = _guarded(K * B); bq, vq = _guarded((n + 1) * B); bP, vP = _guarded(nnz_p * B)
    sA = (1, K) if A_layout == "major" else (B, 1)
    sq = (1, n + 1) if q_layout == "major" else (B, 1)
    pst = _struct_dev(struct) if struct is not None else None
    sk = skip.view(torch.uint8) if skip is not None else None
    t = [xa, ya, xb, yb] if torch.is_tensor(xa) else [_cuda(v) for v in (xa, ya, xb, yb)]
    rc = _lib.lib().ce_lpgd_grad(eng._h, B, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), float(delta), sk.data_ptr() if sk is not None else None,
                                 vA.data_ptr(), *sA, vq.data_ptr(), *sq, vP.data_ptr() if nnz_p else None, pst[0].data_ptr() if pst else None,
                                 pst[1].data_ptr() if pst else None, nnz_p, eng._stream())
    _lib.check(rc, "ce_lpgd_grad")
    torch.cuda.synchronize()
    assert _guards_intact(bA, K * B) and _guards_intact(bq, (n + 1) * B) and _guards_intact(bP, nnz_p * B), "a guard band was written"
    dA = (vA.view(B, K).t() if A_layout == "major" else vA.view(K, B)).cpu().numpy()
    dq = (vq.view(B, n + 1).t() if q_layout == "major" else vq.view(n + 1, B)).cpu().numpy()
    return dA, dq, (vP.view(B, nnz_p).cpu().numpy() if nnz_p else None)


def _exact_grad(tpl, xa, ya, xb, yb, delta, struct=None):
    """the staged form in longdouble, boundary convention: (dA, dq, dP) and the sum of the absolute values of the staged terms of each, divided by delta"""
    xa, ya, xb, yb = (np.asarray(v, LD) for v in (xa, ya, xb, yb))
    B, n = xa.shape
    rows, cols = vk.entries(tpl)
    Dx, Dy = xb - xa, yb - ya
    is_A = cols < n
    cA = np.where(is_A, cols, 0)
    t1 = np.where(is_A[None], yb[:, rows] * Dx[:, cA], Dy[:, rows])
    t2 = np.where(is_A[None], Dy[:, rows] * xa[:, cA], 0)
    dA, sA = (-(t1 + t2) / delta).T, ((np.abs(t1) + np.abs(t2)) / delta).T
    dq = np.concatenate([Dx / delta, np.zeros((B, 1), LD)], axis=1).T
    dP = sP = None
    if struct is not None:
        pr, pc, w = vk.p_entries(struct)
        p1, p2 = xb[:, pr] * Dx[:, pc], Dx[:, pr] * xa[:, pc]
        dP, sP = LD(w)[None] * (p1 + p2) / delta, w[None] * (np.abs(p1) + np.abs(p2)) / delta
    return (dA, dq, dP), (sA, np.abs(dq), sP)


def _assert_staged(got, exact, scale, what):
    err = np.abs(np.asarray(got, np.float64).astype(LD) - exact).astype(float)
    tol = 8.0 * U * np.asarray(scale, np.float64)
    worst = float((err / np.maximum(tol, np.finfo(float).tiny)).max()) if err.size else 0.0
    print(f"{what}: max error / bound = {worst:.3f} over {err.size} entries")
    assert (err <= tol).all(), (what, worst)


def _points(B, n, m, seed):
    rng = np.random.default_rng(seed)
    xa, ya = rng.standard_normal((B, n)), rng.standard_normal((B, m))
    return xa, ya, xa + 0.05 * rng.standard_normal((B, n)), ya + 0.05 * rng.standard_normal((B, m))


@pytest.mark.parametrize("B", [1, 3, 5, 63, 65, 130])
def test_grad_equals_the_staged_numpy_form_in_both_layouts(B):
    """B at the edges of the four-instance workgroup of the batch-major kernel and of the 64-instance tile of the batch-minor one; every third instance of the
    larger batches is skipped with NaN in every input: exact zeros there, the neighbours unchanged bit for bit"""
    n, cones = lk.SOC_SHAPE
    tpl = P.dense_template(n, cones)
    eng = _engine(tpl)
    xa, ya, xb, yb = _points(B, n, tpl.m, 10 + B)
    delta = 0.2
    (w_dA, w_dq, _), (s_dA, s_dq, _) = _exact_grad(tpl, xa, ya, xb, yb, delta)
    skip = torch.zeros(B, dtype=torch.bool, device=DEV); skip[::3] = True; skip[B - 1] = True
    sk = skip.cpu().numpy()
    bad = [_cuda(v).clone() for v in (xa, ya, xb, yb)]
    for t in bad:
        t[skip] = float("nan")
    for A_layout, q_layout in (("major", "major"), ("minor", "minor"), ("major", "minor"), ("minor", "major")):
        dA, dq, _ = _raw_grad(eng, xa, ya, xb, yb, delta, A_layout=A_layout, q_layout=q_layout)
        _assert_staged(dA, w_dA, s_dA, f"dA {A_layout}"); _assert_staged(dq, w_dq, s_dq, f"dq {q_layout}")
        assert (dq[n] == 0).all()
        dA_s, dq_s, _ = _raw_grad(eng, *bad, delta, skip=skip, A_layout=A_layout, q_layout=q_layout)
        assert (dA_s[:, sk] == 0).all() and (dq_s[:, sk] == 0).all() and not np.isnan(dA_s).any() and not np.isnan(dq_s).any()
        assert np.array_equal(dA_s[:, ~sk], dA[:, ~sk]) and np.array_equal(dq_s[:, ~sk], dq[:, ~sk])


def test_grad_sparse_template_with_structural_zeros_in_b():
    tpl, B = _template("sparse_b65")
    eng = _engine(tpl)
    xa, ya, xb, yb = _points(B, tpl.n, tpl.m, 5)
    (w_dA, w_dq, _), (s_dA, s_dq, _) = _exact_grad(tpl, xa, ya, xb, yb, 0.02)
    for layout in ("major", "minor"):
        dA, dq, _ = _raw_grad(eng, xa, ya, xb, yb, 0.02, A_layout=layout, q_layout=layout)
        _assert_staged(dA, w_dA, s_dA, f"dA {layout}"); _assert_staged(dq, w_dq, s_dq, f"dq {layout}")


def test_grad_staged_tiles_split_over_several_chunks_of_entries():
    """the metric shape (n = 50, m = 100, 5100 entries): a staged tile is served by several workgroups, each with its own chunk of the entries; B = 65 has a
    full and a one-instance tile"""
    cfg = P.CONFIGS["M"]
    tpl = P.dense_template(cfg["n"], cfg["cones"])
    assert tpl.nnz_aug > 4096 and 2 * 65 * (tpl.n + tpl.m) * 8 < 159 * 1024
    eng = _engine(tpl)
    B = 65
    xa, ya, xb, yb = _points(B, tpl.n, tpl.m, 8)
    (w_dA, w_dq, _), (s_dA, s_dq, _) = _exact_grad(tpl, xa, ya, xb, yb, 0.1)
    skip = torch.zeros(B, dtype=torch.bool, device=DEV); skip[[5, 64]] = True
    sk = skip.cpu().numpy()
    bad = [_cuda(v).clone() for v in (xa, ya, xb, yb)]
    for t in bad:
        t[skip] = float("nan")
    for layout in ("minor", "major"):
        dA, dq, _ = _raw_grad(eng, xa, ya, xb, yb, 0.1, A_layout=layout, q_layout=layout)
        _assert_staged(dA, w_dA, s_dA, f"dA {layout}"); _assert_staged(dq, w_dq, s_dq, f"dq {layout}")
        dA_s, dq_s, _ = _raw_grad(eng, *bad, 0.1, skip=skip, A_layout=layout, q_layout=layout)
        assert (dA_s[:, sk] == 0).all() and (dq_s[:, sk] == 0).all()
        assert np.array_equal(dA_s[:, ~sk], dA[:, ~sk]) and np.array_equal(dq_s[:, ~sk], dq[:, ~sk])


def test_grad_gathers_from_global_memory_when_a_tile_exceeds_lds():
    """the construction of test_gpu_value.py::test_tile_kernel_gathers_from_global_memory_when_a_tile_exceeds_lds: n + m = 350; the staged tile of this kernel holds
    four vectors per instance (2 * 65 * 350 * 8 bytes > 160 KiB), so its lanes gather"""
    n, cones, B = 200, {"z": 0, "l": 150, "q": []}, 65
    rng = np.random.default_rng(3)
    pattern = rng.random((150, n)) < 0.05
    tpl = P.dense_template(n, cones, pattern=pattern)
    assert 2 * 65 * (n + tpl.m) * 8 > 160 * 1024
    eng = _engine(tpl)
    xa, ya, xb, yb = _points(B, n, tpl.m, 6)
    (w_dA, w_dq, _), (s_dA, s_dq, _) = _exact_grad(tpl, xa, ya, xb, yb, 0.1)
    skip = torch.zeros(B, dtype=torch.bool, device=DEV); skip[[2, 64]] = True
    sk = skip.cpu().numpy()
    bad = [_cuda(v).clone() for v in (xa, ya, xb, yb)]
    for t in bad:
        t[skip] = float("nan")
    for layout in ("major", "minor"):
        dA, dq, _ = _raw_grad(eng, xa, ya, xb, yb, 0.1, A_layout=layout, q_layout=layout)
        _assert_staged(dA, w_dA, s_dA, f"dA {layout}"); _assert_staged(dq, w_dq, s_dq, f"dq {layout}")
        dA_s, dq_s, _ = _raw_grad(eng, *bad, 0.1, skip=skip, A_layout=layout, q_layout=layout)
        assert (dA_s[:, sk] == 0).all() and (dq_s[:, sk] == 0).all()
        assert np.array_equal(dA_s[:, ~sk], dA[:, ~sk]) and np.array_equal(dq_s[:, ~sk], dq[:, ~sk])


@pytest.mark.parametrize("kind", ["full", "one_triangle"])
def test_grad_of_P_in_a_symmetric_and_a_one_triangle_structure(kind):
    from qp_ns_kit import full_structure
    from test_quad_objective import _upper_structure
    n, cones, B, seed = vk.QP_SHAPE
    struct = full_structure(n) if kind == "full" else _upper_structure(n)
    assert vk.one_triangle(*vk.p_entries(struct)[:2]) == (kind == "one_triangle")
    tpl = P.dense_template(n, cones)
    xa, ya, xb, yb = _points(B, n, tpl.m, seed)
    (w_dA, w_dq, w_dP), (s_dA, s_dq, s_dP) = _exact_grad(tpl, xa, ya, xb, yb, 0.3, struct)
    for eng in (_engine(tpl), _engine(tpl, struct)):
        for layout in ("major", "minor"):
            dA, dq, dP = _raw_grad(eng, xa, ya, xb, yb, 0.3, A_layout=layout, q_layout=layout, struct=struct)
            _assert_staged(dA, w_dA, s_dA, "dA"); _assert_staged(dq, w_dq, s_dq, "dq"); _assert_staged(dP, w_dP, s_dP, "dP")
        skip = torch.zeros(B, dtype=torch.bool, device=DEV); skip[1] = True
        bad = [_cuda(v).clone() for v in (xa, ya, xb, yb)]
        for t in bad:
            t[1] = float("nan")
        dA_s, dq_s, dP_s = _raw_grad(eng, *bad, 0.3, skip=skip, struct=struct)
        keep = np.arange(B) != 1
        assert (dP_s[1] == 0).all() and (dA_s[:, 1] == 0).all() and (dq_s[:, 1] == 0).all()
        assert np.array_equal(dP_s[keep], _raw_grad(eng, xa, ya, xb, yb, 0.3, struct=struct)[2][keep])


def test_bad_arguments_are_refused_before_any_launch():
    tpl, B = _template("dense_b5")
    eng = _engine(tpl)
    xa, ya, xb, yb = (_cuda(v) for v in _points(B, tpl.n, tpl.m, 1))
    out = torch.empty((B, tpl.nnz_aug), dtype=torch.float64, device=DEV)
    L = _lib.lib()
    assert L.ce_lpgd_grad(eng._h, B, xa.data_ptr(), ya.data_ptr(), xb.data_ptr(), yb.data_ptr(), 0.0, None, out.data_ptr(), 1, tpl.nnz_aug, None, 0, 0, None, None, None, 0, eng._stream()) == -1
    assert L.ce_lpgd_grad(eng._h, B, xa.data_ptr(), ya.data_ptr(), xb.data_ptr(), yb.data_ptr(), 0.1, None, out.data_ptr(), 3, 2, None, 0, 0, None, None, None, 0, eng._stream()) == -1
    q = torch.zeros((tpl.n + 1, B), dtype=torch.float64, device=DEV)
    fl = torch.zeros(B, dtype=torch.int32, device=DEV)
    # dy without an A output
    assert L.ce_lpgd_perturb(eng._h, B, None, 0, q.data_ptr(), B, 1, None, None, None, 0, xa.data_ptr(), xa.data_ptr(), ya.data_ptr(), 0.1, 0.0, q.data_ptr(), None, None, fl.data_ptr(), eng._stream()) == -1
    assert L.ce_lpgd_perturb(eng._h, B, None, 0, q.data_ptr(), B, 1, None, None, None, 0, xa.data_ptr(), xa.data_ptr(), None, 0.0, 0.0, q.data_ptr(), None, None, fl.data_ptr(), eng._stream()) == -1

"""k_newton_wave_qp (ce_jvp_qp_wave, ce_refine_qp_wave): the forward derivative and one Newton refinement step of a small template with a quadratic objective
inside the kernels, one instance per wave, at the planted KKT points of tests/test_gpu_bwd_wave_qp.py (SHAPES, case(): ns_edge_kit.plant, kind "qp", B = 24, seed 3)
against ns_edge_kit's dense references with P.  Every planted instance is regular (cond(J) <= 6.0e5, KKT residual <= 6e-16) and both references accept all 24
instances of all twelve shapes, so none is left out: the forward derivative's bound is case()'s max(1e-9, 10 (n + m) 2^-53 max cond(J)) (the same matrix J), the
refinement's is tests/test_gpu_ns_mode_edges.py's 10 d_ref + _refine_floor (d_start 5e-6 to 1.1e-5, d_ref <= 1.4e-9), the transpose identity's
tests/test_gpu_newton_wave.py's 1e-6."""
import numpy as np
import pytest
import torch

import ns_edge_kit as K
import qp_ns_kit as Q
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from test_gpu_bwd_wave_qp import B, SHAPES, case
from test_gpu_ns_mode_edges import _refine_floor, _rel
from test_quad_objective import _upper_structure

pytestmark = pytest.mark.gpu
_T: dict = {}
CASES = [(name, False) for name in SHAPES] + [("row1_full", True)]


def tangent(name, triangle=False, duplicate_row=False):
    """case() of the key with what the forward block needs beside it: the planted point again (plant is deterministic; the duplicated row as case() writes it),
    q_eval, Gaussian tangents (tP symmetric) on the device and the two dense references' inputs: built once per key, shared, not changed"""
    key = (name, triangle, duplicate_row)
    if key not in _T:
        (n, cones, states), kw = SHAPES[name]
        pt = dict(K.plant(("qp", n, cones, states), B=B, seed=3, **kw))
        if duplicate_row:
            A, b = pt["A"].copy(), pt["b"].copy()
            A[1::2, 1] = A[1::2, 0]; b[1::2, 1] = b[1::2, 0]
            pt.update(A=A, b=b, c=-np.einsum("bij,bj->bi", pt["Pm"], pt["x"]) - np.einsum("bij,bi->bj", A, pt["y"]))
        tpl = P.dense_template(n, cones)
        struct = _upper_structure(n) if triangle else Q.full_structure(n)
        t = K.tangents(pt)
        tA_eval, tq_eval = tpl.values_from_dense(*t[:3])
        _T[key] = dict(case(name, triangle, duplicate_row), pt=pt, q=Q.device_values(tpl, pt["A"], pt["b"], pt["c"], pt["Pm"], struct)[1],
                       tA=torch.from_numpy(tA_eval).cuda().t().contiguous(), tq=torch.from_numpy(tq_eval).cuda(),
                       tP=torch.from_numpy(Q.p_tangent_values(t[3], struct)).cuda(), want=K.dense_jvp(pt, t))
    return _T[key]


def jvp(c, tA, tq, tP, sel=slice(None), wave=True):
    A, x, y, s = (t[sel].contiguous() for t in c["dev"][:4])
    cut = lambda t, col=False: None if t is None else (t[:, sel] if col else t[sel]).contiguous()
    out = c["eng"].jvp(A, x, y, s, cut(tA), cut(tq, True), path="per_instance", method="direct", P_bm=c["P_bm"][sel].contiguous(), tP_bm=cut(tP), wave=wave)
    return (*out, c["eng"].last_lsqr_iters)


def refine(c, start, sel=slice(None)):
    xt, yt, st = (torch.from_numpy(a).cuda()[sel].contiguous() for a in start[:3])
    x, y, s, info = c["eng"].refine(c["dev"][0][sel].contiguous(), c["q"][:, sel].contiguous(), xt, yt, st, 1, status=None, P_bm=c["P_bm"][sel].contiguous(), wave=True)
    return x, y, s, info["status"], torch.stack([info["resid_before"], info["resid_after"]], dim=1), info


@pytest.mark.parametrize("name,triangle", CASES)
def test_forward_derivative_against_the_dense_solve(name, triangle):
    c = tangent(name, triangle)
    assert c["eng"].newton_wave_qp_plan()[0] == c["eng"].bwd_wave_qp_plan()[0] >= 0
    dx, dy, ds, st, its = jvp(c, c["tA"], c["tq"], c["tP"])
    assert c["eng"].last_jvp_kernel == "ce_jvp_qp_wave"
    torch.cuda.synchronize()
    assert c["want"][3].all()
    e = np.max([_rel(g.cpu().numpy(), w) for g, w in zip((dx, dy, ds), c["want"][:3])], axis=0)
    print(f"{name}{' (one triangle)' if triangle else ''}: forward derivative max {e.max():.3e} (bound {c['bound']:.1e}) status {np.bincount(st.cpu().numpy()).tolist()}")
    assert (st.cpu().numpy() == 0).all() and (its.cpu().numpy() == 0).all()
    assert (e < c["bound"]).all(), e
    z = jvp(c, None, None, None)
    assert all((g == 0).all() for g in z[:3]) and (z[3] == 0).all()          # null tangents: exact zeros
    p = jvp(c, None, None, c["tP"])
    assert (p[3] == 0).all() and max(float(p[0].abs().max()), float(p[1].abs().max())) > 1e-3          # a tangent in P alone moves the solution (nf = 0: y alone)
    # the transpose identity with the wave adjoint at the same points: <xb, dx> + <yb, dy> = <dA, tA> + <dq, tq> + <dP, tP>
    dA, dq, adj, dP = c["eng"].vjp(*c["dev"], path="per_instance", P_bm=c["P_bm"], wave=True)
    xb, yb = c["dev"][4], c["dev"][5]
    lhs = ((xb * dx).sum(dim=1) + (yb * dy).sum(dim=1)).cpu().numpy()
    rhs = ((dA.t() * c["tA"]).sum(dim=1) + (dq * c["tq"]).sum(dim=0) + (dP * c["tP"]).sum(dim=1)).cpu().numpy()
    ti = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
    print(f"{name}: transpose identity max {ti.max():.3e} (bound 1e-6)")
    assert (adj.cpu().numpy() == 0).all() and (ti < 1e-6).all() and np.abs(lhs).max() > 1e-3, ti


@pytest.mark.parametrize("name,triangle", CASES)
def test_one_refinement_step(name, triangle):
    c = tangent(name, triangle)
    pt = c["pt"]
    start = K.perturbed(pt)
    x, y, s, rst, resid, info = refine(c, start)
    assert info["path"] == "ns" and info["kernel"] == "k_newton_wave_qp"
    torch.cuda.synchronize()
    rst, (r0, r1) = rst.cpu().numpy(), resid.cpu().numpy().T
    xr, vr, ok = K.dense_newton(pt, start[0], start[3])
    assert ok.all()
    d_start, d_ref, d_gpu = K.distance(pt, start[0], start[3]), K.distance(pt, xr, vr), K.distance(pt, x.cpu().numpy(), (y - s).cpu().numpy())
    print(f"{name}: status {np.bincount(rst).tolist()} distance start {d_start.max():.3e} reference {d_ref.max():.3e} kernel {d_gpu.max():.3e}; rho {r0.max():.3e} -> {r1.max():.3e}")
    assert (r1 <= r0).all(), (r0, r1)
    assert ((rst & 1) == 1).all() and ((rst & (4 | 16)) == 0).all() and (info["steps"].cpu().numpy() == 1).all(), rst
    bound = 10 * d_ref + _refine_floor(pt, d_start)
    assert (d_gpu <= bound).all(), (d_gpu, bound)


def test_an_instance_does_not_depend_on_its_position():
    c = tangent("row1_full")
    start = K.perturbed(c["pt"])
    perm = torch.from_numpy(np.random.default_rng(5).permutation(B)).cuda()
    inv = torch.argsort(perm)
    for run in (lambda sel: jvp(c, c["tA"], c["tq"], c["tP"], sel)[:4], lambda sel: refine(c, start, sel)[:5]):          # dx, dy, ds, status | x, y, s, status, resid
        base, got, one = run(slice(None)), run(perm), run(slice(5, 6))
        for b_, g_, o_ in zip(base, got, one):
            assert torch.equal(g_[inv], b_) and torch.equal(o_[0], b_[5])


def test_a_redundant_equality_row_is_flagged():
    c = tangent("row1_full", duplicate_row=True)
    odd = np.arange(B) % 2 == 1
    dx, dy, ds, st, its = jvp(c, c["tA"], c["tq"], c["tP"])
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == np.where(odd, 4, 0)).all() and (its.cpu().numpy() == 0).all(), (st, its)          # 4, never 4 | 8: no LSQR has a P term
    assert all(bool(torch.isfinite(g).all()) for g in (dx, dy, ds))
    want = c["want"]          # (the dense solve leaves the singular odd instances out)
    e = np.max([_rel(g.cpu().numpy()[~odd], w[~odd]) for g, w in zip((dx, dy, ds), want[:3])], axis=0)
    print(f"even instances: forward derivative max {e.max():.3e} (bound {c['bound']:.1e})")
    assert want[3][~odd].all() and (e < c["bound"]).all()
    start = K.perturbed(c["pt"])
    x, y, s, rst, _, _ = refine(c, start)
    rst = rst.cpu().numpy()
    assert ((rst[odd] & 4) == 4).all() and ((rst[odd] & 1) == 0).all() and ((rst[~odd] & 4) == 0).all(), rst
    for a, g in zip(start[:3], (x, y, s)):
        assert np.array_equal(a[odd], g.cpu().numpy()[odd])


def test_refusals_leave_the_outputs_untouched():
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    L = _lib.lib()
    tpl = P.dense_template(16, dict(z=2, l=10, q=[4, 16]))
    lin = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))
    big = Q.qp_engine(P.dense_template(33, dict(z=1, l=4, q=[])), Q.full_structure(33))
    f64 = dict(dtype=torch.float64, device="cuda")
    for eng, why in ((lin, "without a P structure"), (big, "n > 32")):
        assert eng.newton_wave_qp_plan() == (-1, 0)
        z = torch.zeros((2, eng.nnz_aug + max(eng.nnz_p, 1) + eng.n + eng.m), **f64)
        out, iout = torch.full((2, eng.n + eng.m), 7.0, **f64), torch.full((2,), 7, dtype=torch.int32, device="cuda")
        p, o, io = z.data_ptr(), out.data_ptr(), iout.data_ptr()
        for entry in ("ce_jvp_qp_wave", "ce_refine_qp_wave"):
            if entry == "ce_jvp_qp_wave":
                rc = L.ce_jvp_qp_wave(eng._h, 2, p, eng.nnz_aug, p, p, p, p, p, eng.nnz_aug, None, 0, 0, p, o, o, o, io, io, None)
            else:
                rc = L.ce_refine_qp_wave(eng._h, 2, p, eng.nnz_aug, p, 2, 1, p, o, o, o, None, 1, io, io, o, None)
            torch.cuda.synchronize()
            msg = L.ce_last_error().decode()
            assert rc == -2 and entry in msg and why in msg, (rc, msg)
            assert (out == 7).all() and (iout == 7).all()
    with pytest.raises(NotImplementedError, match="ce_jvp_qp_wave"):
        big.jvp(*(torch.zeros((2, k), **f64) for k in (big.nnz_aug, big.n, big.m, big.m)), None, None, path="per_instance", method="direct",
                P_bm=torch.zeros((2, big.nnz_p), **f64), wave=True)
    with pytest.raises(NotImplementedError, match="ce_refine_qp_wave"):
        big.refine(torch.zeros((2, big.nnz_aug), **f64), torch.zeros((big.n + 1, 2), **f64), *(torch.zeros((2, k), **f64) for k in (big.n, big.m, big.m)), 1,
                   P_bm=torch.zeros((2, big.nnz_p), **f64), wave=True)

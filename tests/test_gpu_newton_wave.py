"""k_newton_wave (ce_jvp_wave, ce_refine_wave): the forward derivative and one Newton refinement step of a small template, one instance per wave, at the planted
KKT points of tests/test_gpu_bwd_wave.py (SHAPES, case(): ns_edge_kit.plant, kind "plain", B = 24, seed 3) against ns_edge_kit's dense references.  Every planted
instance is regular (cond(J) <= 3.3e3, KKT residual <= 1e-15) and both references accept every instance, so none is left out: the forward derivative's bound is
that file's 1e-9 = cond 3.3e3 x 2^-53 x (n + m = 96) x 10 (the same matrix J), the refinement's is tests/test_gpu_ns_mode_edges.py's 10 d_ref + _refine_floor."""
import numpy as np
import pytest
import torch

import ns_edge_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_bwd_wave import B, BOUND, SHAPES, case
from test_gpu_ns_mode_edges import _refine_floor, _rel

pytestmark = pytest.mark.gpu
_T: dict = {}


def tangent(name, duplicate_row=False):
    """the Gaussian tangents of a case on the device and the dense reference: built once per name, shared, not changed"""
    key = (name, duplicate_row)
    if key not in _T:
        c = case(name, duplicate_row)
        t = K.tangents(c["pt"])
        tA_eval, tq_eval = c["tpl"].values_from_dense(*t[:3])
        _T[key] = dict(tA=torch.from_numpy(tA_eval).cuda().t().contiguous(), tq=torch.from_numpy(tq_eval).cuda(), want=K.dense_jvp(c["pt"], t))
    return _T[key]


def jvp(c, tA, tq, sel=slice(None), **kw):
    A, x, y, s = (t[sel].contiguous() for t in c["dev"][:4])
    out = c["eng"].jvp(A, x, y, s, None if tA is None else tA[sel].contiguous(), None if tq is None else tq[:, sel].contiguous(), path="per_instance", lsqr=TIGHT_LSQR,
                       q_eval=c["q"][:, sel].contiguous(), method="direct", **kw)
    return (*out, c["eng"].last_lsqr_iters)


def refine(c, start, sel=slice(None), **kw):
    xt, yt, st = (torch.from_numpy(a).cuda()[sel].contiguous() for a in start[:3])
    x, y, s, info = c["eng"].refine(c["dev"][0][sel].contiguous(), c["q"][:, sel].contiguous(), xt, yt, st, 1, status=None, **kw)
    return x, y, s, info["status"], torch.stack([info["resid_before"], info["resid_after"]], dim=1), info


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_derivative_against_the_dense_solve(name):
    c, t = case(name), tangent(name)
    assert c["eng"].newton_wave_plan()[0] == c["eng"].bwd_wave_plan()[0] >= 0
    dx, dy, ds, st, its = jvp(c, t["tA"], t["tq"], wave=True)
    assert c["eng"].last_jvp_kernel == "ce_jvp_wave"
    torch.cuda.synchronize()
    assert t["want"][3].all()
    e = np.max([_rel(g.cpu().numpy(), w) for g, w in zip((dx, dy, ds), t["want"][:3])], axis=0)
    print(f"{name}: forward derivative max {e.max():.3e} (bound {BOUND:.0e}) status {np.bincount(st.cpu().numpy()).tolist()}")
    assert (st.cpu().numpy() == 0).all() and (its.cpu().numpy() == 0).all()
    assert e.max() < BOUND, e
    z = jvp(c, None, None, wave=True)
    assert all((g == 0).all() for g in z[:3]) and (z[3] == 0).all()          # null tangents: exact zeros
    # the transpose identity with the wave adjoint at the same points: <xb, dx> + <yb, dy> = <dA, tA> + <dq, tq>
    dA, dq, adj = c["eng"].vjp(*c["dev"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"], wave=True)
    xb, yb = c["dev"][4], c["dev"][5]
    lhs = ((xb * dx).sum(dim=1) + (yb * dy).sum(dim=1)).cpu().numpy()
    rhs = ((dA.t() * t["tA"]).sum(dim=1) + (dq * t["tq"]).sum(dim=0)).cpu().numpy()
    ti = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
    print(f"{name}: transpose identity max {ti.max():.3e} (bound 1e-6)")
    assert (adj.cpu().numpy() == 0).all() and (ti < 1e-6).all() and np.abs(lhs).max() > 1e-3, ti


@pytest.mark.parametrize("name", list(SHAPES))
def test_one_refinement_step(name):
    c = case(name)
    pt = c["pt"]
    start = K.perturbed(pt)
    x, y, s, rst, resid, info = refine(c, start, wave=True)
    assert info["path"] == "ns" and info["kernel"] == "k_newton_wave"
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
    c, t = case("row1_full"), tangent("row1_full")
    start = K.perturbed(c["pt"])
    perm = torch.from_numpy(np.random.default_rng(5).permutation(B)).cuda()
    inv = torch.argsort(perm)
    for run in (lambda sel: jvp(c, t["tA"], t["tq"], sel, wave=True)[:4], lambda sel: refine(c, start, sel, wave=True)[:5]):          # dx, dy, ds, status | x, y, s, status, resid
        base, got, one = run(slice(None)), run(perm), run(slice(5, 6))
        for b_, g_, o_ in zip(base, got, one):
            assert torch.equal(g_[inv], b_) and torch.equal(o_[0], b_[5])


def test_a_redundant_equality_row_is_flagged():
    c, t = case("row1_full", duplicate_row=True), tangent("row1_full", duplicate_row=True)
    odd = np.arange(B) % 2 == 1
    odd_t = torch.from_numpy(odd).cuda()
    dx, dy, ds, st, its = jvp(c, t["tA"], t["tq"], wave=True)
    ref = jvp(c, t["tA"], t["tq"])
    assert c["eng"].last_jvp_kernel == "ce_jvp"
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == np.where(odd, 12, 0)).all() and (its.cpu().numpy()[odd] > 0).all() and (its.cpu().numpy()[~odd] == 0).all(), (st, its)
    for g, r in zip((dx, dy, ds, st, its), ref):          # the same LSQR launch re-solves them: the same bits
        assert torch.equal(g[odd_t], r[odd_t])
    even = ~odd
    want = t["want"]          # (the dense solve leaves the singular odd instances out: they are LSQR's above)
    e = np.max([_rel(g.cpu().numpy()[even], w) for g, w in zip((dx, dy, ds), (w[even] for w in want[:3]))], axis=0)
    print(f"even instances: forward derivative max {e.max():.3e} (bound {BOUND:.0e})")
    assert want[3][even].all() and e.max() < BOUND
    start = K.perturbed(c["pt"])
    x, y, s, rst, _, _ = refine(c, start, wave=True)
    rst = rst.cpu().numpy()
    assert ((rst[odd] & 4) == 4).all() and ((rst[odd] & 1) == 0).all() and ((rst[~odd] & 4) == 0).all(), rst
    for a, g in zip(start[:3], (x, y, s)):
        assert np.array_equal(a[odd], g.cpu().numpy()[odd])


def test_refusals_leave_the_outputs_untouched():
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    c, L = case("row1_full"), _lib.lib()
    tpl = P.dense_template(4, dict(z=0, l=3, q=[], ep=1, p=[]))
    exp_eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))
    assert exp_eng.newton_wave_plan() == (-1, 0)
    f64 = dict(dtype=torch.float64, device="cuda")
    for entry, eng, q, why in (("ce_jvp_wave", exp_eng, c["q"], "exponential"), ("ce_refine_wave", exp_eng, c["q"], "exponential"), ("ce_jvp_wave", c["eng"], None, "q_vals == NULL")):
        z = torch.zeros((2, eng.nnz_aug + eng.n + eng.m), **f64)
        out, iout = torch.full((2, eng.nnz_aug + eng.m), 7.0, **f64), torch.full((2,), 7, dtype=torch.int32, device="cuda")
        q_args = (q.data_ptr(), 2, 1) if q is not None else (None, 0, 0)
        p, o, io = z.data_ptr(), out.data_ptr(), iout.data_ptr()
        if entry == "ce_jvp_wave":
            rc = L.ce_jvp_wave(eng._h, 2, p, eng.nnz_aug, *q_args, p, p, p, p, eng.nnz_aug, None, 0, 0, o, o, o, io, io, 1e-8, 1e-8, 1e8, 0, None)
        else:
            rc = L.ce_refine_wave(eng._h, 2, p, eng.nnz_aug, *q_args, o, o, o, None, 1, io, io, o, None)
        torch.cuda.synchronize()
        msg = L.ce_last_error().decode()
        assert rc != 0 and entry in msg and why in msg, (rc, msg)
        assert (out == 7).all() and (iout == 7).all()
    with pytest.raises(NotImplementedError, match="ce_jvp_wave"):
        exp_eng.jvp(*(torch.zeros((2, k), **f64) for k in (exp_eng.nnz_aug, exp_eng.n, exp_eng.m, exp_eng.m)), None, None, path="per_instance",
                    q_eval=torch.zeros((exp_eng.n + 1, 2), **f64), method="direct", wave=True)

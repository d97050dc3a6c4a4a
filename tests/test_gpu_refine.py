"""Newton refinement of solutions on the search-free elimination: k_backward_ns<..., FWD, REF> behind ce_refine, ConeEngine.refine, solver_args refine_steps.
The starting point is the engine's own solve at eps = 1e-4 (computed once per shape and never changed: every refinement works on clones).  Checked against
  * the forward derivative by direct elimination (ce_jvp) fed the residual as its tangent -- the same system, another prologue and epilogue;
  * a dense numpy Newton step on [[0, A^T D], [A, D - I]];
  * the oracle at eps = 1e-11 (the converged share, the points, the gradients through the layer);
  * the safeguard: rho never grows, rejected / flagged / failed instances keep their point bit for bit.
rho, y-hat, s-hat as include/cone_engine.h ce_refine states them."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import ref_cases
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_jvp import _engine, _tangents
from test_gpu_jvp_direct import SHAPES as _JVP_SHAPES

pytestmark = pytest.mark.gpu

# shape -> (n, cones, B, seed): test_gpu_jvp_direct.SHAPES with its seeds and batch sizes (all three variants of the kernel, the single-wave and the multi-wave
# row elimination) and a nonnegative-only program
ALL = {k: v[:4] for k, v in _JVP_SHAPES.items()}
ALL["lp"] = (20, {"z": 0, "l": 40, "q": []}, 48, 6)
_CACHE: dict = {}


def _proj(v, cones):
    """projection of one v onto the dual cone (zero -> free, nonnegative, second-order) and its derivative D"""
    z, l, q = cones.get("z", 0), cones.get("l", 0), cones.get("q", [])
    out = v.copy(); m = v.size; D = np.zeros((m, m))
    D[np.arange(z), np.arange(z)] = 1.0
    for i in range(z, z + l):
        out[i] = max(v[i], 0.0); D[i, i] = 1.0 if v[i] > 0 else 0.0
    o = z + l
    for d in q:
        t, w = v[o], v[o + 1:o + d]; nz = np.linalg.norm(w)
        if d == 1:
            out[o] = max(t, 0.0); D[o, o] = 1.0 if t >= 0 else 0.0
        elif nz <= t:
            D[o:o + d, o:o + d] = np.eye(d)
        elif nz <= -t:
            out[o:o + d] = 0.0
        else:
            a = (t + nz) / 2; wh = w / nz
            out[o] = a; out[o + 1:o + d] = a * wh
            Dm = np.zeros((d, d)); Dm[0, 0] = 0.5; Dm[0, 1:] = wh / 2; Dm[1:, 0] = wh / 2
            Dm[1:, 1:] = ((t + nz) / (2 * nz)) * np.eye(d - 1) - (t / (2 * nz)) * np.outer(wh, wh)
            D[o:o + d, o:o + d] = Dm
        o += d
    return out, D


def _residual(A, b, c, x, v, cones):
    """(F_x, F_y, y-hat, D) of one instance at (x, v)"""
    yh, D = _proj(v, cones)
    return A.T @ yh + c, A @ x + (yh - v) - b, yh, D


def _rho(A, b, c, x, y, s):
    """rho of every instance at the arrays as given, in extended precision (the error of the comparison is then the kernel's own)"""
    L = np.longdouble
    A, b, c, x, y, s = (np.asarray(t, dtype=L) for t in (A, b, c, x, y, s))
    fx = np.einsum("bij,bi->bj", A, y) + c; fy = np.einsum("bij,bj->bi", A, x) + s - b
    num = np.maximum(np.abs(fx).max(axis=1), np.abs(fy).max(axis=1))
    return (num / (1 + np.maximum(np.abs(b).max(axis=1), np.abs(c).max(axis=1)))).astype(np.float64)


def _solve_start(tpl, A, b, c, **args):
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = _engine(tpl)
    A_bm = torch.from_numpy(A_eval).cuda().t().contiguous(); q_t = torch.from_numpy(q_eval).cuda()
    x, y, s, _, status, _ = eng.solve(A_bm, q_t, make_settings(dict(eps=1e-4, **args)))
    torch.cuda.synchronize()
    return dict(tpl=tpl, eng=eng, A=A, b=b, c=c, A_bm=A_bm, q_t=q_t, pt=(x, y, s), status=status, np=tuple(t.cpu().numpy() for t in (x, y, s)))


def _refine(r, steps, status="given"):
    """(x, y, s, status, steps, resid_before, resid_after) as numpy arrays of `steps` steps from the start (clones: the start stays what it is)"""
    x, y, s = (t.clone() for t in r["pt"])
    x, y, s, info = r["eng"].refine(r["A_bm"], r["q_t"], x, y, s, steps, status=r["status"] if isinstance(status, str) else status)
    assert info["path"] == "ns"
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (x, y, s, info["status"], info["steps"], info["resid_before"], info["resid_after"]))


def _shape(name):
    """the shape's problem, its eps = 1e-4 start on the GPU, one and three refinement steps from it, the oracle at eps = 1e-11: computed once, shared, not changed"""
    if name not in _CACHE:
        from oracle import oracle
        n, cones, B, seed = ALL[name]
        tpl = P.dense_template(n, cones)
        A, b, c = P.generate(n, cones, B, seed=seed)
        r = _solve_start(tpl, A, b, c)
        assert (r["status"].cpu().numpy() > 0).all(), r["status"]
        r["cones"] = cones
        r["one"], r["three"] = _refine(r, 1), _refine(r, 3)
        r["hi"] = oracle.solve_batch(A, b, c, cones, eps=1e-11, max_iters=200000)
        _CACHE[name] = r
    return _CACHE[name]


def _step_errors(r, dx_ref, dv_ref, sel):
    """per selected instance: max(|x+ - x - dx|, |v+ - v - dv|) relative to the instance's max |dx|"""
    x0, y0, s0 = r["np"]; x1, y1, s1 = r["one"][:3]
    ex = np.abs((x1 - x0) - dx_ref).max(axis=1); ev = np.abs(((y1 - s1) - (y0 - s0)) - dv_ref).max(axis=1)
    return (np.maximum(ex, ev) / np.abs(dx_ref).max(axis=1))[sel]


def _check_step_bounds(e, what):
    """the bounds the elimination is held to against LSQR in test_gpu_jvp_direct.py, scale-free"""
    print(f"{what}: {e.size} instances, max {e.max():.3e} median {np.median(e):.3e}")
    assert e.max() < 1e-5 and np.median(e) < 1e-8, (what, e.max(), np.median(e))


@pytest.mark.parametrize("shape", list(ALL))
def test_one_step_is_the_direct_jvp_with_the_residual_as_tangent(shape):
    r = _shape(shape)
    tpl, eng, A, b, c = r["tpl"], r["eng"], r["A"], r["b"], r["c"]
    if shape in _JVP_SHAPES and _JVP_SHAPES[shape][4] is not None:
        assert _lib.lib().ce_adjoint_ns_variant(eng._h) == _JVP_SHAPES[shape][4]
    x0, y0, s0 = r["np"]
    B = x0.shape[0]
    gx = np.zeros((B, tpl.n)); gy = np.zeros((B, tpl.m))
    for i in range(B):
        fx, fy, _, _ = _residual(A[i], b[i], c[i], x0[i], y0[i] - s0[i], r["cones"])
        gx[i], gy[i] = fx, -fy
    tA = np.zeros((B, tpl.nnz_aug)); tA[:, tpl.nnzA + np.arange(tpl.b_idx.size)] = gy[:, tpl.b_idx]
    tq = np.zeros((tpl.n + 1, B)); tq[:tpl.n] = gx.T
    dx, dy, ds, jst = eng.jvp(r["A_bm"], *r["pt"], torch.from_numpy(tA).cuda(), torch.from_numpy(tq).cuda(), path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    assert eng.last_jvp_kernel == "ce_jvp"
    torch.cuda.synchronize()
    dx, dy, ds, jst = (t.cpu().numpy() for t in (dx, dy, ds, jst))
    st = r["one"][3]
    kept = (st & 1) != 0
    print("kept", kept.mean(), "refine status counts", np.bincount(st), "jvp status counts", np.bincount(jst))
    assert kept.mean() >= 0.9          # (the cap of the convergence test: an instance that converges in three steps kept its first)
    assert (jst[kept] == 0).all()          # the same elimination flags the same instances
    assert ((st & 4) != 0)[jst != 0].all()
    _check_step_bounds(_step_errors(r, dx, dy - ds, kept), "one step vs ce_jvp")


@pytest.mark.parametrize("shape", list(ALL))
def test_one_step_is_a_dense_newton_step(shape):
    r = _shape(shape)
    A, b, c, cones = r["A"], r["b"], r["c"], r["cones"]
    x0, y0, s0 = r["np"]
    B, n = x0.shape; m = y0.shape[1]
    dxr = np.zeros((B, n)); dvr = np.zeros((B, m)); ok = np.zeros(B, bool); acc = np.zeros(B, bool)
    for i in range(B):
        v = y0[i] - s0[i]
        fx, fy, _, D = _residual(A[i], b[i], c[i], x0[i], v, cones)
        J = np.block([[np.zeros((n, n)), A[i].T @ D], [A[i], D - np.eye(m)]])
        if not np.isfinite(J).all() or np.linalg.cond(J) > 1e11:
            continue
        d = np.linalg.solve(J, -np.concatenate([fx, fy]))
        ok[i] = True; dxr[i], dvr[i] = d[:n], d[n:]
        fxn, fyn, _, _ = _residual(A[i], b[i], c[i], x0[i] + d[:n], v + d[n:], cones)
        acc[i] = max(np.abs(fxn).max(), np.abs(fyn).max()) < max(np.abs(fx).max(), np.abs(fy).max())
    st = r["one"][3]
    kept = (st & 1) != 0
    print("well conditioned", ok.mean(), "reference accepts", acc[ok].mean(), "kernel kept", kept[ok].mean())
    both = ok & acc & kept
    assert both.mean() >= 0.8, both.mean()
    _check_step_bounds(_step_errors(r, dxr, dvr, both), "one step vs numpy")


@pytest.mark.parametrize("shape", list(ALL))
def test_three_steps_converge_to_the_oracle_point(shape):
    """CPU prototype from the oracle's eps = 1e-4 point: share >= 0.99 on every shape, x within 4e-10; the 0.9 leaves room for the engine's different iterate.
    Shares measured on the MI355X are in DESIGN.md 3.3."""
    r = _shape(shape)
    x, y, s, st, taken, r0, r1 = r["three"]
    cones, hi = r["cones"], r["hi"]
    conv = r1 <= 1e-12
    print(f"{shape}: share with resid_after <= 1e-12: {conv.mean():.3f}; status counts {np.bincount(st)}; steps kept {np.bincount(taken)}; "
          f"resid before median {np.median(r0):.2e}, after median {np.median(r1):.2e} max {r1.max():.2e}")
    assert conv.mean() >= 0.9, conv.mean()
    cmp_ = conv & (hi["status"] == 1)
    assert cmp_.mean() >= 0.9
    for name, got in zip("xys", (x, y, s)):
        e = (np.abs(got - hi[name]).max(axis=1) / (1 + np.abs(hi[name]).max(axis=1)))[cmp_]
        print(f"  {name}: max rel error against the oracle {e.max():.2e}")
        assert e.max() < 1e-8, (name, e.max())
    rn = _rho(r["A"], r["b"], r["c"], x, y, s)
    print(f"  rho recomputed / reported: min {np.min(rn / np.maximum(r1, 1e-300)):.3f} max {np.max(rn / np.maximum(r1, 1e-300)):.3f}, max abs difference {np.abs(rn - r1).max():.2e}")
    assert (((rn <= 2 * r1) & (r1 <= 2 * rn)) | (np.abs(rn - r1) <= 1e-15)).all(), (rn, r1)
    # y+ in K*, s+ in K, complementary.  Zero-cone and nonnegative rows are exact by construction (s = y - v with y = v or y = 0); a second-order block is
    # lam (|z|, z) and its difference with v: each entry carries a few ulp of the block's largest entry, d <= 11 of them enter a norm -> 1e-13 (1 + max |.|)
    z, l = cones.get("z", 0), cones.get("l", 0)
    assert (s[:, :z] == 0).all() and (y[:, z:z + l] >= 0).all() and (s[:, z:z + l] >= 0).all()
    o = z + l
    for d in cones.get("q", []):
        for w in (y, s):
            blk = w[:, o:o + d]
            assert (blk[:, 0] - np.linalg.norm(blk[:, 1:], axis=1) >= -1e-13 * (1 + np.abs(blk).max(axis=1))).all()
        o += d
    ys = np.abs((y * s).sum(axis=1))
    assert (ys <= 1e-12 * (1 + np.linalg.norm(y, axis=1) * np.linalg.norm(s, axis=1)))[conv].all(), ys.max()


def _assert_never_worse(start, out):
    """rho of the returned point <= rho of the one that came in; an instance that kept no step has its point bit for bit; an instance the forward solve failed on
    is skipped (bit 16 alone, no rho evaluated: NaN)"""
    x, y, s, st, taken, r0, r1 = out
    skipped = (st & 16) != 0
    assert (st[skipped] == 16).all() and np.isnan(r0[skipped]).all() and np.isnan(r1[skipped]).all()
    assert (r1 <= r0)[~skipped].all(), (r0, r1)
    assert ((taken > 0) == ((st & 1) != 0)).all()
    same = (st & 1) == 0
    for a, b in zip(start, (x, y, s)):
        assert np.array_equal(a[same], b[same], equal_nan=True)
    moved = ~same
    assert (r1[moved] < r0[moved]).all()
    return st


@pytest.mark.parametrize("shape", list(ALL))
@pytest.mark.parametrize("steps", ["one", "three"])
def test_never_worse(shape, steps):
    r = _shape(shape)
    st = _assert_never_worse(r["np"], r[steps])
    assert ((st & 16) == 0).all() and ((st & 7) != 0).all()          # every instance took a step, was rejected or was flagged
    rn = _rho(r["A"], r["b"], r["c"], *r[steps][:3])
    r0 = r[steps][5]
    assert (rn <= r0 * (1 + 1e-9) + 1e-15).all()          # ... and rho recomputed in extended precision agrees that nothing grew (to the rounding of the kernel's own sums)


def test_duplicated_equality_rows_are_flagged_and_left_alone():
    """the mutation of test_gpu_jvp_direct.py: every second instance has a redundant equality row; the row elimination flags it (bit 4), no step is taken"""
    n, cones, B = 12, {"z": 4, "l": 8, "q": [5]}, 24
    A, b, c = P.generate(n, cones, B, seed=11)
    deg = np.arange(B) % 2 == 0
    A[deg, 2, :] = A[deg, 0, :]; b[deg, 2] = b[deg, 0]
    r = _solve_start(P.dense_template(n, cones), A, b, c)
    out = _refine(r, 3)
    st = _assert_never_worse(r["np"], out)
    solved = r["status"].cpu().numpy() >= 0          # (the forward solve at eps = 1e-4 gives up on some of the degenerate instances: those are skipped, as test_gpu_jvp_direct.py leaves them out)
    print("forward status", r["status"].cpu().numpy(), "refine status", st)
    assert solved.mean() >= 0.8 and (solved == ((st & 16) == 0)).all()
    assert (st[deg & solved] == 4).all() and ((st[~deg] & 4) == 0).all(), st
    for a, g in zip(r["np"], out[:3]):
        assert np.array_equal(a[deg], g[deg], equal_nan=True)
    assert ((st[~deg & solved] & 1) != 0).mean() >= 0.9
    # without the forward status every duplicated-row instance reaches the elimination: all of them carry bit 4 and keep their point
    out_all = _refine(r, 3, status=None)
    assert ((out_all[3][deg] & 4) != 0).all() and ((out_all[3][deg] & 1) == 0).all() and (out_all[4][deg] == 0).all(), out_all[3]
    for a, g in zip(r["np"], out_all[:3]):
        assert np.array_equal(a[deg], g[deg], equal_nan=True)


def test_never_worse_from_a_25_iteration_start():
    cfg = P.CONFIGS["M"]; n, cones, B = cfg["n"], cfg["cones"], 48
    A, b, c = P.generate(n, cones, B, seed=3)
    r = _solve_start(P.dense_template(n, cones), A, b, c, max_iters=25)
    out = _refine(r, 3, status=None)
    st = _assert_never_worse(r["np"], out)
    print("status counts", np.bincount(st), "resid before median", np.median(out[5]), "after median", np.median(out[6]))
    assert ((st & 16) == 0).all()
    rn = _rho(A, b, c, *out[:3])
    assert (rn <= out[5] * (1 + 1e-9) + 1e-15).all()


def _lp_layer_inputs():
    n, cones, B = 6, {"z": 2, "l": 10}, 4
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=4)
    return n, cones, B, tpl, A, b, c


def test_failed_instances_are_skipped_and_masked_as_before():
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    n, cones, B, tpl, A, b, c = _lp_layer_inputs()
    A[0, 2, :] = 0.0; b[0, 2] = -1.0          # a nonnegative row  0 x + s = -1: infeasible
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    ctx = MI355_ctx(None, tpl.problem_data_index, cones, options={"eps": 1e-4, "raise_on_error": False})
    A_t, q_t = torch.from_numpy(A_eval).cuda(), torch.from_numpy(q_eval).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p0, d0, info0, _ = _CvxpyLayer.apply(None, q_t, A_t, ctx, {}, True, None)
        p1, d1, info1, _ = _CvxpyLayer.apply(None, q_t, A_t, ctx, {"refine_steps": 2}, True, None)
    torch.cuda.synchronize()
    assert info1["status"].cpu().numpy()[0] < 0 and "refine" not in info0
    for a, g in zip((p0, d0), (p1, d1)):
        assert torch.isnan(a[0]).all() and torch.isnan(g[0]).all() and torch.isfinite(g[1:]).all()
    st = info1["refine"]["status"].cpu().numpy()
    print("refine status", st, "resid", info1["refine"]["resid_before"].cpu().numpy(), info1["refine"]["resid_after"].cpu().numpy())
    assert info1["refine"]["path"] == "ns" and st[0] == 16 and ((st[1:] & 1) != 0).all(), st
    assert (info1["refine"]["resid_after"][1:] < info1["refine"]["resid_before"][1:]).all()
    assert not torch.equal(p0[1:], p1[1:])


def test_off_means_off():
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    n, cones, B, tpl, A, b, c = _lp_layer_inputs()
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    ctx = MI355_ctx(None, tpl.problem_data_index, cones, options={"eps": 1e-4})
    w = torch.from_numpy(np.random.default_rng(2).standard_normal((B, n))).cuda()
    got = []
    for args in ({}, {"refine_steps": 0}):
        A_t, q_t = torch.from_numpy(A_eval).cuda().requires_grad_(), torch.from_numpy(q_eval).cuda().requires_grad_()
        primal, dual, info, _ = _CvxpyLayer.apply(None, q_t, A_t, ctx, args, True, None)
        (primal * w).sum().backward()
        assert "refine" not in info
        got.append((primal.detach(), dual.detach(), A_t.grad, q_t.grad))
    for a, g in zip(*got):
        assert torch.equal(a, g)


def _identity_layer(n, cones, args):
    from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    m = P.cone_rows(cones)
    tpl = template_from_affine_builder(lambda A, b, c: (A, b, c), [(m, n), (m,), (n,)], cones, [VariableRecovery(slice(0, n), None, (n,))])
    return CvxpyLayer(template=tpl, solver_args=args)


def test_gradients_at_the_refined_point_are_the_oracles():
    """backward through cvxpylayers_amd.torch.CvxpyLayer at eps = 1e-4 + three steps against the oracle's dense adjoint at its eps = 1e-11 point (prototype: <= 7e-10
    where converged); the same comparison without refinement misses by more than 1e-3 somewhere -- what the feature changes"""
    from oracle import oracle
    n, cones, B, seed = ALL["v0_single_wave"]
    A, b, c = P.generate(n, cones, B, seed=seed)
    hi = oracle.solve_batch(A, b, c, cones, eps=1e-11, max_iters=200000)
    w = np.random.default_rng(5).standard_normal((B, n))
    ref = oracle.adjoint_batch(A, b, c, cones, hi["x"], hi["y"], hi["s"], w, np.zeros_like(hi["y"]), mode="dense")

    def errors(args):
        layer = _identity_layer(n, cones, args)
        ps = [torch.from_numpy(t).cuda().requires_grad_() for t in (A, b, c)]
        (x,) = layer(*ps)
        (x * torch.from_numpy(w).cuda()).sum().backward()
        torch.cuda.synchronize()
        e = np.zeros(B)
        for p_, k in zip(ps, ("dA", "db", "dc")):
            g = p_.grad.cpu().numpy().reshape(B, -1); want = ref[k].reshape(B, -1)
            e = np.maximum(e, np.abs(g - want).max(axis=1) / (1 + np.abs(want).max(axis=1)))
        return e, layer.info
    e1, info = errors({"eps": 1e-4, "refine_steps": 3})
    conv = (info["refine"]["resid_after"].cpu().numpy() <= 1e-12) & (hi["status"] == 1)
    print(f"converged {conv.mean():.3f}; refined gradients: max {e1[conv].max():.3e} median {np.median(e1[conv]):.3e}")
    assert info["refine"]["path"] == "ns" and conv.mean() >= 0.9
    assert e1[conv].max() < 1e-6, e1[conv].max()
    e0, info0 = errors({"eps": 1e-4})
    print(f"unrefined gradients: max {e0.max():.3e} median {np.median(e0):.3e}")
    assert "refine" not in info0 and e0.max() > 1e-3


def test_forward_ad_through_the_refined_layer_against_central_differences():
    """recipe and bound of test_gpu_jvp.py::test_jvp_is_the_derivative_of_the_gpu_solution_map (h = 1e-5, 2e-4 (1 + max |jvp|)); the differences are taken of
    the layer at eps = 1e-10, the tangent comes from the layer at eps = 1e-4 + three steps with jvp_mode="direct" """
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    n, cones, B = 12, {"z": 2, "l": 10, "q": [4, 5]}, 8
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=7)
    ctx = MI355_ctx(None, tpl.problem_data_index, cones, options={"acceleration_lookback": 0})
    (dA, db, dc), tA_bm, tq = _tangents(tpl, B, seed=3)

    def values(A_, b_, c_):
        A_eval, q_eval = tpl.values_from_dense(A_, b_, c_)
        return torch.from_numpy(A_eval).cuda(), torch.from_numpy(q_eval).cuda()
    A_t, q_t = values(A, b, c)
    with fwAD.dual_level():
        primal, dual, info, _ = _CvxpyLayer.apply(None, fwAD.make_dual(q_t, tq), fwAD.make_dual(A_t, tA_bm.t()), ctx, {"eps": 1e-4, "refine_steps": 3, "jvp_mode": "direct"}, True, None)
        tp, td = (fwAD.unpack_dual(t).tangent.cpu().numpy() for t in (primal, dual))
    assert info["jvp"]["path"] == "direct" and info["refine"]["path"] == "ns"
    conv = info["refine"]["resid_after"].cpu().numpy() <= 1e-12
    print("converged", conv, "jvp status", info["jvp"]["status"].cpu().numpy())
    assert conv.sum() >= 7          # (0.9 of 8 instances)
    h = 1e-5
    fd = []
    for sgn in (1.0, -1.0):
        Ah, qh = values(A + sgn * h * dA, b + sgn * h * db, c + sgn * h * dc)
        p_, d_, inf_, _ = _CvxpyLayer.apply(None, qh, Ah, ctx, {"eps": 1e-10, "max_iters": 200000}, False, None)
        fd.append((p_.cpu().numpy(), d_.cpu().numpy()))
    for name, an, k in (("dx", tp, 0), ("dy", td, 1)):
        d = (fd[0][k] - fd[1][k]) / (2 * h)
        err = np.abs(d - an)[conv].max()
        print(f"{name}: max |jvp - fd| = {err:.3e}, max |jvp| = {np.abs(an[conv]).max():.3e}")
        assert err < 2e-4 * (1 + np.abs(an[conv]).max()), (name, err)


def test_templates_without_the_elimination_keep_their_point_and_say_so_once(monkeypatch):
    from cvxpylayers_amd.interfaces import mi355_if
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    from cvxpylayers_amd.torch import CvxpyLayer
    mi355_if._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        # a PSD template through the frontend
        cs = ref_cases.case_sdp_symmetric_primal_and_psd_dual()
        (C0,) = (torch.from_numpy(p).cuda() for p in cs["params"])
        layer = CvxpyLayer(template=cs["template"], solver_args={"eps": 1e-4})
        plain = [o.clone() for o in layer(C0)]
        assert "refine" not in layer.info
        ref = [o.clone() for o in layer(C0, solver_args={"refine_steps": 2})]
        assert layer.info["refine"]["path"] == "none" and layer.info["refine"]["status"] is None
        assert all(torch.equal(a, g) for a, g in zip(plain, ref))
        # a shared-A template on the shared-A path
        B = 6
        A, b, c, cones, tpl = P.portfolio_c5_batch(B, seed=3, nw=60, kf=9)
        Ab = np.broadcast_to(A, (B,) + A.shape).copy(); bb = np.broadcast_to(b, (B,) + b.shape).copy()
        monkeypatch.setenv("CE_CONST_A", "1")
        A_eval, q_eval = tpl.values_from_dense(Ab, bb, c)
        ctx = MI355_ctx(None, tpl.problem_data_index, cones, options={"eps": 1e-4})
        A_t, q_t = torch.from_numpy(A_eval).cuda(), torch.from_numpy(q_eval).cuda()
        p0, d0, info0, _ = _CvxpyLayer.apply(None, q_t, A_t, ctx, {}, True, None)
        p1, d1, info1, _ = _CvxpyLayer.apply(None, q_t, A_t, ctx, {"refine_steps": 2}, True, None)
        eng = ctx.engine(torch.device("cuda", 0))
        assert eng.last_path == "const_a" and info1["refine"]["path"] == "none" and "refine" not in info0
        assert torch.equal(p0, p1) and torch.equal(d0, d1)
    said = [w for w in rec if "refine_steps" in str(w.message)]
    assert len(said) == 1, [str(w.message) for w in rec]
    # the library's own refusal on a PSD engine
    eng = _engine(P.dense_template(4, {"z": 1, "s": [3]}))
    assert _lib.lib().ce_adjoint_ns_variant(eng._h) < 0
    Bp = 3
    zf = torch.zeros((Bp, max(eng.n, eng.m, eng.nnz_aug)), dtype=torch.float64, device="cuda"); zi = torch.zeros((Bp,), dtype=torch.int32, device="cuda")
    q0 = torch.zeros((eng.n + 1, Bp), dtype=torch.float64, device="cuda")
    rc = _lib.lib().ce_refine(eng._h, Bp, zf.data_ptr(), eng.nnz_aug, q0.data_ptr(), q0.stride(0), q0.stride(1), zf.data_ptr(), zf.data_ptr(), zf.data_ptr(), None, 2,
                              zi.data_ptr(), zi.data_ptr(), zf.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -2 and b"search-free" in _lib.lib().ce_last_error()


def test_unbatched_call_and_a_batch_of_one():
    from cvxpylayers_amd.torch import CvxpyLayer
    from test_gpu_jvp import _closed_form
    cs = ref_cases.case_ridge_unbatched()
    layer = CvxpyLayer(template=cs["template"], solver_args={"eps": 1e-4, "refine_steps": 3})
    F0, g0 = (torch.from_numpy(p).cuda() for p in cs["params"])
    (x,) = layer(F0, g0)
    rf = layer.info["refine"]
    st = rf["status"].cpu().numpy()
    print("unbatched: status", st, "resid", rf["resid_before"].cpu().numpy(), rf["resid_after"].cpu().numpy())
    assert x.shape == (F0.shape[1],) and st.shape == (1,) and rf["path"] == "ns"
    assert (rf["resid_after"] <= rf["resid_before"]).all()
    assert (rf["resid_after"] <= 1e-12).all()          # converged: the closed form to the oracle's accuracy bound of the convergence test
    want = _closed_form(F0, g0)
    print("unbatched: max |x - closed form|", float((x - want).abs().max()))
    assert (x - want).abs().max() < 1e-8 * (1 + want.abs().max()), (x - want).abs().max()
    # B = 1 at the engine: the instance does what it does inside its batch, bit for bit
    r = _shape("v0_small")
    x1, y1, s1 = (t[:1].clone() for t in r["pt"])
    x1, y1, s1, info = r["eng"].refine(r["A_bm"][:1].contiguous(), r["q_t"][:, :1].contiguous(), x1, y1, s1, 3, status=r["status"][:1])
    torch.cuda.synchronize()
    assert info["path"] == "ns" and int(info["status"][0]) == int(r["three"][3][0])
    for got, want in zip((x1, y1, s1), r["three"][:3]):
        assert np.array_equal(got.cpu().numpy()[0], want[0])

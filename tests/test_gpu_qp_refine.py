"""Newton refinement of templates whose quadratic objective runs inside the kernels: k_backward_ns<..., FWD, REF, QP> behind ce_refine_qp, ConeEngine.refine(P_bm=),
solver_args refine_steps on the native-QP route.  Mirrors test_gpu_refine.py with F_x = P x + A^T y^ + c: the start is the engine's own eps = 1e-4 QP point (computed
once per shape, never changed), checked against
  * ce_jvp_qp fed the residual as its tangent -- the same system, another prologue and epilogue -- and a dense numpy Newton step on [[P, A^T D], [A, D - I]]
    (bounds of test_gpu_refine.py: 1e-5 maximum, 1e-8 median, relative to the instance's max |dx|, beyond the rounding of the stored points: _step_errors);
  * the oracle's QP solve at eps = 1e-11: share with resid_after <= 1e-12 >= 0.9 after three steps, x, y, s within 1e-8 there, cone membership, complementarity;
  * the safeguard: rho never grows for 1, 2, 3 steps, also from a 25-iteration start; flagged / failed instances keep their point bit for bit;
  * gradients (dA, dq, dP) at the refined eps = 1e-4 point against the oracle's at eps = 1e-11 (1e-6 where converged)."""
import warnings

import numpy as np
import pytest
import torch

import qp_ns_kit as K
from cvxpylayers_amd import problems as P
from test_gpu_refine import _assert_never_worse, _check_step_bounds
from test_quad_objective import _p_values, _upper_structure

pytestmark = pytest.mark.gpu

SHAPES = ["small_mixed", "metric", "box_qp", "row2_n80", "inactive_box"]
_CACHE: dict = {}


def _step_errors(r, dx_ref, dv_ref, sel):
    """test_gpu_refine.py::_step_errors -- per selected instance max(|x+ - x - dx|, |v+ - v - dv|) relative to the instance's max |dx| -- beyond what fp64 can
    represent of a step that is read back as a DIFFERENCE of stored points (u = 2^-53):  x+ = fl(x + dx) is off by at most u |x+|;  v+ = fl(v + fl(dy - ds)) by
    u (|v+| + |dv|), and it is stored as y+ = Pi(v+), s+ = fl(y+ - v+) and read as fl(y+ - s+), two more roundings of entries no larger than max(|y+|, |s+|) (exact on
    zero-cone and nonnegative rows).  With |v| <= |y| + |s| that is at most 6 u max(|x|, |y|, |s|) over both points, whatever the kernel does; it is subtracted, the
    raw figure is printed.  Where max |dx| > 1e-7 of the point the allowance is below a hundredth of the median bound and the check is test_gpu_refine.py's; it
    matters where the start is converged already: the box that is nowhere active is an unconstrained quadratic which the eps = 1e-4 solve leaves at rho = 1.5e-12, so
    max |dx| ~ 1e-13 of x and the rounding of x+ alone is 1e-4 of the step."""
    x0, y0, s0 = r["np"]; x1, y1, s1 = r["one"][:3]
    ex = np.abs((x1 - x0) - dx_ref).max(axis=1); ev = np.abs(((y1 - s1) - (y0 - s0)) - dv_ref).max(axis=1)
    scale = np.max([np.abs(t).max(axis=1) for t in (x0, y0, s0, x1, y1, s1)], axis=0)
    raw = np.maximum(ex, ev); allow = 6 * 2.0 ** -53 * scale
    nd = np.abs(dx_ref).max(axis=1)
    print(f"  raw step error / max|dx|: max {(raw / nd)[sel].max():.3e} median {np.median((raw / nd)[sel]):.3e}; fp64 allowance / max|dx|: max {(allow / nd)[sel].max():.3e}; "
          f"max|dx| / max|point|: min {(nd / scale)[sel].min():.3e}")
    return (np.maximum(raw - allow, 0.0) / nd)[sel]


def _problem(name):
    if name == "box_qp":
        return K.box_qp()
    if name == "inactive_box":
        return K.inactive_box()
    n, cones, A, b, c, Pm = K.instance(name)
    return cones, A, b, c, Pm, P.dense_template(n, cones)


def _solve_start(tpl, A, b, c, Pm, **args):
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    struct = _upper_structure(tpl.n)
    eng = K.qp_engine(tpl, struct)
    A_bm, q_t, P_bm = K.device_values(tpl, A, b, c, Pm, struct)
    x, y, s, _, status, _ = eng.solve(A_bm, q_t, make_settings(dict(eps=1e-4, **args)), P_bm=P_bm)
    torch.cuda.synchronize()
    return dict(tpl=tpl, struct=struct, eng=eng, A=A, b=b, c=c, Pm=Pm, A_bm=A_bm, q_t=q_t, P_bm=P_bm, pt=(x, y, s), status=status, np=tuple(t.cpu().numpy() for t in (x, y, s)))


def _refine(r, steps, status="given"):
    x, y, s = (t.clone() for t in r["pt"])
    x, y, s, info = r["eng"].refine(r["A_bm"], r["q_t"], x, y, s, steps, status=r["status"] if isinstance(status, str) else status, P_bm=r["P_bm"])
    assert info["path"] == "ns"
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (x, y, s, info["status"], info["steps"], info["resid_before"], info["resid_after"]))


def _shape(name):
    """the shape's problem, its eps = 1e-4 start on the GPU, one / two / three steps from it, the oracle at eps = 1e-11: computed once, shared, not changed"""
    if name not in _CACHE:
        from oracle import oracle
        cones, A, b, c, Pm, tpl = _problem(name)
        r = _solve_start(tpl, A, b, c, Pm)
        assert (r["status"].cpu().numpy() > 0).all(), r["status"]
        r["cones"] = cones
        r["one"], r["two"], r["three"] = _refine(r, 1), _refine(r, 2), _refine(r, 3)
        r["hi"] = oracle.solve_batch(A, b, c, cones, P=Pm, eps=1e-11, max_iters=200000)
        _CACHE[name] = r
    return _CACHE[name]


@pytest.mark.parametrize("shape", SHAPES)
def test_one_step_is_the_qp_jvp_with_the_residual_as_tangent(shape):
    r = _shape(shape)
    tpl, eng, A, b, c, Pm = r["tpl"], r["eng"], r["A"], r["b"], r["c"], r["Pm"]
    x0, y0, s0 = r["np"]
    B = x0.shape[0]
    gx = np.zeros((B, tpl.n)); gy = np.zeros((B, tpl.m))
    for i in range(B):
        fx, fy, _, _ = K.qp_residual(A[i], b[i], c[i], Pm[i], x0[i], y0[i] - s0[i], r["cones"])
        gx[i], gy[i] = fx, -fy
    assert tpl.b_idx.size == tpl.m          # (every row has a b entry: the whole of g_y can be fed as a tangent of b)
    tA = np.zeros((B, tpl.nnz_aug)); tA[:, tpl.nnzA + np.arange(tpl.b_idx.size)] = gy[:, tpl.b_idx]
    tq = np.zeros((tpl.n + 1, B)); tq[:tpl.n] = gx.T
    dx, dy, ds, jst = eng.jvp(r["A_bm"], *r["pt"], torch.from_numpy(tA).cuda(), torch.from_numpy(tq).cuda(), method="direct", P_bm=r["P_bm"], tP_bm=None)
    assert eng.last_jvp_kernel == "ce_jvp_qp"
    torch.cuda.synchronize()
    dx, dy, ds, jst = (t.cpu().numpy() for t in (dx, dy, ds, jst))
    st = r["one"][3]
    kept = (st & 1) != 0
    print("kept", kept.mean(), "refine status counts", np.bincount(st), "jvp status counts", np.bincount(jst))
    assert kept.mean() >= 0.9
    assert (jst[kept] == 0).all()          # the same elimination flags the same instances
    assert ((st & 4) != 0)[jst != 0].all()
    _check_step_bounds(_step_errors(r, dx, dy - ds, kept), "one step vs ce_jvp_qp")


@pytest.mark.parametrize("shape", SHAPES)
def test_one_step_is_a_dense_newton_step(shape):
    r = _shape(shape)
    A, b, c, Pm, cones = r["A"], r["b"], r["c"], r["Pm"], r["cones"]
    x0, y0, s0 = r["np"]
    B, n = x0.shape; m = y0.shape[1]
    dxr = np.zeros((B, n)); dvr = np.zeros((B, m)); ok = np.zeros(B, bool); acc = np.zeros(B, bool)
    for i in range(B):
        v = y0[i] - s0[i]
        fx, fy, _, _ = K.qp_residual(A[i], b[i], c[i], Pm[i], x0[i], v, cones)
        J, _ = K.kkt_matrix(A[i], Pm[i], v, cones)
        if not np.isfinite(J).all() or np.linalg.cond(J) > 1e11:
            continue
        d = np.linalg.solve(J, -np.concatenate([fx, fy]))
        ok[i] = True; dxr[i], dvr[i] = d[:n], d[n:]
        fxn, fyn, _, _ = K.qp_residual(A[i], b[i], c[i], Pm[i], x0[i] + d[:n], v + d[n:], cones)
        acc[i] = max(np.abs(fxn).max(), np.abs(fyn).max()) < max(np.abs(fx).max(), np.abs(fy).max())
    st = r["one"][3]
    kept = (st & 1) != 0
    print("well conditioned", ok.mean(), "reference accepts", acc[ok].mean(), "kernel kept", kept[ok].mean())
    both = ok & acc & kept
    assert both.mean() >= 0.8, both.mean()
    _check_step_bounds(_step_errors(r, dxr, dvr, both), "one step vs numpy")


@pytest.mark.parametrize("shape", SHAPES)
def test_three_steps_converge_to_the_oracle_point(shape):
    """numpy prototype from the oracle's eps = 1e-4 point: share 1.000 on every shape, x within 1.4e-10; the 0.9 leaves room for the engine's different iterate"""
    r = _shape(shape)
    x, y, s, st, taken, r0, r1 = r["three"]
    cones, hi = r["cones"], r["hi"]
    conv = r1 <= 1e-12
    print(f"{shape}: share with resid_after <= 1e-12: {conv.mean():.3f}; status counts {np.bincount(st)}; steps kept {np.bincount(taken)}; "
          f"resid before median {np.median(r0):.2e}, after median {np.median(r1):.2e} max {r1.max():.2e}")
    assert conv.mean() >= 0.9, conv.mean()
    if shape == "inactive_box":
        assert ((st & 4) == 0).all(), st          # H = 0: regular through P alone
    cmp_ = conv & (hi["status"] == 1)
    assert cmp_.mean() >= 0.9
    for name, got in zip("xys", (x, y, s)):
        e = (np.abs(got - hi[name]).max(axis=1) / (1 + np.abs(hi[name]).max(axis=1)))[cmp_]
        print(f"  {name}: max rel error against the oracle {e.max():.2e}")
        assert e.max() < 1e-8, (name, e.max())
    rn = K.qp_rho(r["A"], r["b"], r["c"], r["Pm"], x, y, s)
    assert (((rn <= 2 * r1) & (r1 <= 2 * rn)) | (np.abs(rn - r1) <= 1e-15)).all(), (rn, r1)
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


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("steps", ["one", "two", "three"])
def test_never_worse(shape, steps):
    r = _shape(shape)
    st = _assert_never_worse(r["np"], r[steps])
    assert ((st & 16) == 0).all() and ((st & 7) != 0).all()
    rn = K.qp_rho(r["A"], r["b"], r["c"], r["Pm"], *r[steps][:3])
    assert (rn <= r[steps][5] * (1 + 1e-9) + 1e-15).all()


def test_never_worse_from_a_25_iteration_start():
    cones, A, b, c, Pm, tpl = _problem("metric")
    r = _solve_start(tpl, A, b, c, Pm, max_iters=25)
    for steps in (1, 2, 3):
        out = _refine(r, steps, status=None)
        st = _assert_never_worse(r["np"], out)
        print(steps, "steps: status counts", np.bincount(st), "resid before median", np.median(out[5]), "after median", np.median(out[6]))
        assert ((st & 16) == 0).all()
        rn = K.qp_rho(A, b, c, Pm, *out[:3])
        assert (rn <= out[5] * (1 + 1e-9) + 1e-15).all()


def test_flagged_instances_keep_their_point():
    """the two flagged fixtures of test_gpu_qp_jvp.py: a repeated zero-cone row in every second instance; a solution set that is not a point (every instance)"""
    n, cones, A, b, c, Pm = K.instance("small_mixed")
    deg = np.arange(A.shape[0]) % 2 == 0
    A[deg, 1, :] = A[deg, 0, :]; b[deg, 1] = b[deg, 0]
    r = _solve_start(P.dense_template(n, cones), A, b, c, Pm)
    out = _refine(r, 3, status=None)
    st = _assert_never_worse(r["np"], out)
    assert (st[deg] == 4).all() and ((st[~deg] & 4) == 0).all(), st
    for a, g in zip(r["np"], out[:3]):
        assert np.array_equal(a[deg], g[deg], equal_nan=True)
    assert ((st[~deg] & 1) != 0).mean() >= 0.9
    B, n = 24, 12
    rng = np.random.default_rng(21)
    G = rng.standard_normal((B, n, n // 2)); Pm = G @ G.transpose(0, 2, 1) / n
    w = rng.standard_normal((B, n)); c = np.einsum("bij,bj->bi", Pm, w)
    A = rng.standard_normal((B, 4, n)); b = -np.einsum("bij,bj->bi", A, w) + 1.0
    cones = {"z": 0, "l": 4, "q": []}
    r = _solve_start(P.dense_template(n, cones), A, b, c, Pm)
    out = _refine(r, 3, status=None)
    st = _assert_never_worse(r["np"], out)
    assert (st == 4).all(), st
    for a, g in zip(r["np"], out[:3]):
        assert np.array_equal(a, g)


def _layer_inputs(B=6):
    from test_quad_objective import _eq_qp
    n, p = 6, 2
    Pm, q, F, g = _eq_qp(n, p, B, seed=1)
    cones = {"z": p, "l": 0, "q": [], "s": []}
    tpl = P.dense_template(n, cones)
    struct = _upper_structure(n)
    A_eval, q_eval = tpl.values_from_dense(F, g, q)
    vals = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (_p_values(Pm, struct).T, q_eval, A_eval)]
    return n, cones, tpl, struct, vals, (Pm, q, F, g)


def test_failed_instances_are_skipped_and_off_means_off():
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    n, cones, tpl, struct, vals, _ = _layer_inputs()
    P_eval, q_eval, A_eval = (v.clone() for v in vals)
    diag = torch.from_numpy(np.flatnonzero(struct[0] == np.repeat(np.arange(n), np.diff(struct[1])))).cuda()
    P_eval[:, 0] = 0.0; P_eval[diag, 0] = 1.0; P_eval[diag[1], 0] = -1.0          # instance 0: indefinite P, the forward solve fails it
    ctx = MI355_ctx(struct, tpl.problem_data_index, cones, options={"eps": 1e-4, "raise_on_error": False})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        p0, d0, info0, _ = _CvxpyLayer.apply(P_eval, q_eval, A_eval, ctx, {}, True, None)
        pz, dz, infoz, _ = _CvxpyLayer.apply(P_eval, q_eval, A_eval, ctx, {"refine_steps": 0}, True, None)
        p1, d1, info1, _ = _CvxpyLayer.apply(P_eval, q_eval, A_eval, ctx, {"refine_steps": 2}, True, None)
    torch.cuda.synchronize()
    assert ctx.engine(torch.device("cuda", 0)).qp_native
    assert "refine" not in info0 and "refine" not in infoz and torch.equal(p0[1:], pz[1:]) and torch.equal(d0[1:], dz[1:])          # off means off
    rf = info1["refine"]
    st = rf["status"].cpu().numpy()
    print("forward status", info1["status"].cpu().numpy(), "refine status", st, "resid", rf["resid_before"].cpu().numpy(), rf["resid_after"].cpu().numpy())
    assert rf["path"] == "ns" and info1["status"].cpu().numpy()[0] < 0 and st[0] == 16 and ((st[1:] & 1) != 0).all(), st
    assert torch.isnan(rf["resid_before"][0]) and torch.isnan(rf["resid_after"][0])
    assert torch.isnan(p1[0]).all() and torch.isfinite(p1[1:]).all()
    assert (rf["resid_after"][1:] < rf["resid_before"][1:]).all() and not torch.equal(p0[1:], p1[1:])


def test_gradients_at_the_refined_point_are_the_oracles():
    """backward through the plugin at eps = 1e-4 + three steps against the oracle's dense QP adjoint at its eps = 1e-11 point: dA, dq, dP within 1e-6 where converged"""
    from oracle import oracle
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    n, cones, A, b, c, Pm = K.instance("small_mixed")
    B = A.shape[0]
    tpl = P.dense_template(n, cones); struct = _upper_structure(n)
    hi = oracle.solve_batch(A, b, c, cones, P=Pm, eps=1e-11, max_iters=200000)
    w = np.random.default_rng(5).standard_normal((B, n))
    g = oracle.adjoint_batch(A, b, c, cones, hi["x"], hi["y"], hi["s"], w, np.zeros_like(hi["y"]), P=Pm, mode="dense")
    cols = np.repeat(np.arange(n + 1), np.diff(tpl.indptr))
    want_A = np.stack([-g["dA"][:, i, j] if j < n else g["db"][:, i] for i, j in zip(tpl.indices, cols)])          # (nnz_aug, B)
    idx, ptr, _ = struct
    pc = np.repeat(np.arange(n), np.diff(ptr))
    want_P = (g["dP"][:, idx, pc] + np.where(idx != pc, g["dP"][:, pc, idx], 0.0)).T          # one stored entry stands for (i, j) and (j, i)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)

    def errors(args):
        ctx = MI355_ctx(struct, tpl.problem_data_index, cones, options={"eps": 1e-4})
        ts = [torch.from_numpy(np.ascontiguousarray(t)).cuda().requires_grad_() for t in (_p_values(Pm, struct).T, q_eval, A_eval)]
        primal, dual, info, _ = _CvxpyLayer.apply(*ts, ctx, args, True, None)
        (primal * torch.from_numpy(w).cuda()).sum().backward()
        torch.cuda.synchronize()
        e = np.zeros(B)
        for t, want in zip(ts, (want_P, g["dc"].T, want_A)):
            got = t.grad.cpu().numpy()[:want.shape[0]]
            e = np.maximum(e, np.abs(got - want).max(axis=0) / (1 + np.abs(want).max(axis=0)))
        return e, info
    e1, info = errors({"refine_steps": 3})
    conv = (info["refine"]["resid_after"].cpu().numpy() <= 1e-12) & (hi["status"] == 1)
    print(f"converged {conv.mean():.3f}; refined gradients: max {e1[conv].max():.3e} median {np.median(e1[conv]):.3e}")
    assert info["refine"]["path"] == "ns" and conv.mean() >= 0.9
    assert e1[conv].max() < 1e-6, e1[conv].max()
    e0, info0 = errors({})
    print(f"unrefined gradients: max {e0.max():.3e} median {np.median(e0):.3e}")
    assert "refine" not in info0 and e0.max() > 1e-6          # (without refinement the same comparison misses the bound: what the feature changes)

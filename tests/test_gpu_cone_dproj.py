"""D Pi_K(v) h of every cone kind on the GPU (ce_cone_dproject behind cvxpylayers_amd/cones.py): against the closed forms at non-kink points, the stated
conventions at kinks, symmetry, torch.autograd.gradcheck in both modes through the public functions, and the handling of the derivative state."""
import numpy as np
import pytest
import torch

from cvxpylayers_amd import cones as CN, problems as P
import cone_proj_kit as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dproj(v, h, cones, dual=False):
    """D Pi(v) h through the wrapper (project with state, then dproject)"""
    cs = CN._cone_set(CN.normalize_cones(cones), DEV)
    vt = _t(v)
    _, state = cs.project(vt, dual, True)
    return cs.dproject(vt, state, _t(h), dual).cpu().numpy()


@pytest.mark.parametrize("B", [1, 2, 65])
def test_rows_and_second_order_cones(B):
    rng = np.random.default_rng(10 + B)
    v = K.rows_soc_input(rng, B); h = rng.standard_normal(v.shape)
    for dual in (False, True):
        out, ref = _dproj(v, h, K.ROWS_SOC, dual), K.rows_soc_dref(v, h, dual=dual)
        assert np.array_equal(out[:, :5], ref[:, :5])
        for a, b in K.soc_spans(K.ROWS_SOC):
            err = np.abs(out[:, a:b] - ref[:, a:b]).max(axis=1)
            assert (err <= 1e-12 * (1 + np.linalg.norm(h[:, a:b], axis=1))).all(), (b - a, err.max())


@pytest.mark.parametrize("orders", K.PSD_ORDERS, ids=lambda o: "s" + "_".join(map(str, o)))
@pytest.mark.parametrize("B", [1, 3])
def test_psd_blocks(orders, B):
    """Within PSD_DPROJ_TOL ||H|| of the eigh closed form: ten times the measured gap (see MEASURED below), never above 1e-11.  The gap is printed."""
    rng = np.random.default_rng(200 * B + orders[0])
    v, mats = K.psd_input(rng, B, orders, "mixed")
    hmats = [rng.standard_normal(S.shape) for S in mats]
    hmats = [0.5 * (H + np.swapaxes(H, 1, 2)) for H in hmats]
    h = np.concatenate([P.sym_to_svec(H) for H in hmats], axis=1)
    out = K.psd_split(_dproj(v, h, {"s": orders}), orders)
    for S, H, D, k in zip(mats, hmats, out, orders):
        for b in range(B):
            gap = np.abs(D[b] - K.psd_dproj(S[b], H[b])).max() / np.linalg.norm(H[b])
            print(f"psd dproj k={k} b={b}: gap {gap:.3e} ||H||")
            assert gap <= PSD_DPROJ_TOL, (k, b, gap)
    for kind, want in (("positive", 1.0), ("negative", 0.0)):          # D Pi = I inside the cone, 0 inside the polar
        v2, _ = K.psd_input(rng, B, orders, kind)
        assert np.abs(_dproj(v2, h, {"s": orders}) - want * h).max() <= 1e-11 * np.abs(h).max(), kind


# MEASURED on an MI355X: the largest gap to the eigh reference over every order and instance above is 1.22e-15 ||H|| (k = 3; 1.21e-15 at k = 17, 1.0e-15 at k = 39,
# 7.3e-16 at k = 40).  The bound is ten times that, far inside the 1e-11 ||H|| that four chained contractions at k <= 40 could cost.
PSD_DPROJ_TOL = 1.3e-14


def test_triples():
    """against oracle.dproj_exp (1e-8) / oracle.dproj_pow (1e-6), the tolerances of tests/test_expcone_host.py"""
    rng = np.random.default_rng(8)
    v = K.triple_points(rng, 200); h = rng.standard_normal(v.shape)
    for dual in (False, True):
        J = K.triples_jac(v, dual=dual)
        out = _dproj(v, h, K.TRIPLES, dual).reshape(200, 4, 3)
        ref = np.einsum("ncij,ncj->nci", J, h.reshape(200, 4, 3))
        scale = 1 + np.abs(h.reshape(200, 4, 3)).sum(axis=2)      # |(J - Jref) h| <= max |J - Jref| sum |h|
        assert (np.abs(out - ref).max(axis=2)[:, :2] <= 1e-8 * scale[:, :2]).all(), dual
        assert (np.abs(out - ref).max(axis=2)[:, 2:] <= 1e-6 * scale[:, 2:]).all(), dual


MIXED = {"z": 2, "l": 3, "q": K.Q_DIMS, "s": [3, 17, 40], "ep": 2, "p": [0.3, -0.6]}


def test_the_derivative_is_symmetric_on_the_mixed_cone_set():
    rng = np.random.default_rng(9)
    B = 9
    v = np.concatenate([K.rows_soc_input(rng, B), K.psd_input(rng, B, MIXED["s"], "mixed")[0], K.triple_points(rng, B)], axis=1)
    g, h = rng.standard_normal(v.shape), rng.standard_normal(v.shape)
    for dual in (False, True):
        Dh, Dg = _dproj(v, h, MIXED, dual), _dproj(v, g, MIXED, dual)
        lhs, rhs = np.sum(g * Dh, axis=1), np.sum(Dg * h, axis=1)
        assert (np.abs(lhs - rhs) <= 1e-12 * np.linalg.norm(g, axis=1) * np.linalg.norm(h, axis=1)).all(), np.abs(lhs - rhs).max()


def test_kink_conventions():
    h = np.array([[1.5, -2.0, 0.25]])
    assert np.array_equal(_dproj(np.array([[0.0, 1.0, -1.0]]), h, {"l": 3}), [[0.75, -2.0, 0.0]])              # a row at exactly 0: factor 1/2
    hq = np.array([[0.3, -1.0, 2.0, 0.5, 0.25, -0.125]])
    on_cone = np.array([[5.0, 3.0, 4.0, 10.0, 6.0, 8.0]])                                                      # t = ||z|| exactly (3-4-5 triangles)
    assert np.array_equal(_dproj(on_cone, hq, {"q": [3, 3]}), hq)                                              # the cone's boundary: the identity
    on_polar = on_cone * np.array([[-1.0, 1.0, 1.0, -1.0, 1.0, 1.0]])
    assert not _dproj(on_polar, hq, {"q": [3, 3]}).any()                                                       # the polar's boundary: 0
    v17, h17 = np.zeros((1, 17)), np.arange(1.0, 18.0)[None]
    v17[0, :3] = (5.0, 3.0, 4.0)
    assert np.array_equal(_dproj(v17, h17, {"q": [17]}), h17)
    v17[0, 0] = -5.0
    assert not _dproj(v17, h17, {"q": [17]}).any()
    # PSD with a zero eigenvalue: it counts as non-positive.  S = diag(2, 0, -1) needs no rotation, so the eigenvalue is an exact 0.
    S = np.diag([2.0, 0.0, -1.0])[None]
    H = np.array([[[1.0, 2.0, 3.0], [2.0, 4.0, 5.0], [3.0, 5.0, 6.0]]])
    Bm = np.array([[1.0, 1.0, 2.0 / 3.0], [1.0, 0.0, 0.0], [2.0 / 3.0, 0.0, 0.0]])
    out = P.svec_to_sym(_dproj(P.sym_to_svec(S), P.sym_to_svec(H), {"s": [3]}), 3)
    assert np.abs(out - Bm * H).max() <= 1e-14


def test_psd_with_two_tiny_eigenvalues_of_opposite_sign():
    rng = np.random.default_rng(11)
    for k in (5, 40):
        Q, _ = np.linalg.qr(rng.standard_normal((k, k)))
        w = K.spectrum("mixed", k); w[0], w[1] = 1e-9, -1e-9
        S = (Q * w) @ Q.T; S = 0.5 * (S + S.T)
        H = rng.standard_normal((k, k)); H = 0.5 * (H + H.T)
        # the closed form from the PRESCRIBED decomposition (eigh of S resolves eigenvalues of 1e-9 to 1e-16 absolute: the same thing to 1e-7)
        ref = Q @ (K.psd_divdiff(w) * (Q.T @ H @ Q)) @ Q.T
        out = P.svec_to_sym(_dproj(P.sym_to_svec(S[None]), P.sym_to_svec(H[None]), {"s": [k]}), k)[0]
        assert np.isfinite(out).all() and np.abs(out - ref).max() <= 1e-6 and np.abs(out - K.psd_dproj(S, H)).max() <= 1e-6


@pytest.mark.parametrize("cones", [{"l": 2, "q": [3]}, {"s": [3]}, {"ep": 1, "p": [0.4]}], ids=["rows_soc", "psd", "triples"])
def test_gradcheck_through_project(cones):
    rng = np.random.default_rng(12)
    if "q" in cones:
        v = K.rows_soc_input(rng, 2, cones)
        v[:, 2] = (0.5, -0.5) * np.linalg.norm(v[:, 3:], axis=1)          # both instances between cone and polar: a curved D Pi
    elif "s" in cones:
        v = K.psd_input(rng, 2, [3], "mixed")[0]
    else:
        v = np.array([[1.0, 0.5, 0.3, 0.4, -0.7, 1.2], [-0.5, 1.0, 0.3, 0.8, 0.3, -1.5]])          # away from every case boundary
    x = _t(v).requires_grad_(True)
    for dual in (False, True):
        assert torch.autograd.gradcheck(lambda t: CN.project(t, cones, dual=dual), (x,), eps=1e-6, atol=1e-6, rtol=1e-5, check_forward_ad=True)


def test_gradcheck_through_project_psd():
    rng = np.random.default_rng(13)
    S = K.psd_matrices(rng, 2, 3, "mixed")[0]
    X = _t(S + 0.1 * np.triu(rng.standard_normal((2, 3, 3)), 1)).requires_grad_(True)          # not symmetric: the gradient is with respect to X itself
    assert torch.autograd.gradcheck(CN.project_psd, (X,), eps=1e-6, atol=1e-6, rtol=1e-5, check_forward_ad=True)


def test_float32_in_float32_out_with_a_gradient_of_the_inputs_dtype():
    v = torch.randn(6, 8, device=DEV, dtype=torch.float32, requires_grad=True)
    out = CN.project(v, {"l": 3, "q": [5]})
    assert out.dtype == torch.float32
    (g,) = torch.autograd.grad(out.sum(), v)
    assert g.dtype == torch.float32 and g.shape == v.shape and torch.isfinite(g).all()


def test_state_is_neither_computed_nor_stored_without_a_gradient():
    cones = {"l": 2, "s": [4], "ep": 1}
    cs = CN._cone_set(CN.normalize_cones(cones), DEV)
    v = torch.randn(3, 2 + 10 + 3, device=DEV, dtype=torch.float64)
    calls, with_state = cs.project_calls, cs.state_calls
    CN.project(v, cones)
    assert (cs.project_calls, cs.state_calls) == (calls + 1, with_state)                       # ce_cone_project received a NULL state
    with torch.no_grad():
        CN.project(v.clone().requires_grad_(True), cones)
    assert (cs.project_calls, cs.state_calls) == (calls + 2, with_state)
    x = v.clone().requires_grad_(True)
    out = CN.project(x, cones)
    assert (cs.project_calls, cs.state_calls) == (calls + 3, with_state + 1)
    w = torch.randn_like(out)
    (g1,) = torch.autograd.grad(out, x, w, retain_graph=True)
    (g2,) = torch.autograd.grad(out, x, w, retain_graph=True)
    assert torch.equal(g1, g2)                                                                 # backward twice: identical gradients
    with torch.autograd.forward_ad.dual_level():
        dual_in = torch.autograd.forward_ad.make_dual(v, w)
        t = torch.autograd.forward_ad.unpack_dual(CN.project(dual_in, cones)).tangent
    assert (cs.project_calls, cs.state_calls) == (calls + 4, with_state + 2) and torch.equal(t, g1)      # D Pi is symmetric: one kernel call serves both modes

"""K tangents at one solution on one factorisation per instance, plain kind: k_backward_ns<..., FWD, ..., MANY> behind ce_jvp_many, ConeEngine.jvp_many.

Shapes, seeds and points are test_gpu_vjp_many.py's (its _point is shared: one oracle solve per shape in a session): small_mixed, ragged_cones, soc_only, M at B = 64,
C3 at B = 8 (the 512-thread variant) and the tile-variant edges n = 28 / 29 / 59 / 60 with its planted points.  K = 1, 3, 17; tangent 0 is repeated at position K - 1
(bit-identical: state left over from one right-hand side to the next would show) and tangent 1 is all zeros (exact zeros on unflagged instances).  Checked against
  * the loop of K jvp(method="direct") calls (force_loop=True): 1e-6 relative to 1 + max |reference| on every instance, equal status and iteration arrays;
  * ce_jvp_lsqr under kit.TIGHT_LSQR on regular instances the reference converged on: 1e-5 worst, 1e-8 median (test_gpu_jvp_direct.py's bounds and its cap: at most
    10 % of the batch left out because the reference did not converge);
  * the transpose identity with vjp_many at the same point, K x K;
  * batch-shared (stride 0) tangents against the same tangents expanded per instance, with only tq, only tA and both: bit for bit;
  * duplicated equality rows and an LP vertex (test_gpu_jvp_direct.py's mutators): 4 | 8 for every k, equal to the loop (an instance listed K times would be re-solved
    K times per tangent and overrun the list of B entries: the loop comparison and the iteration counts are what a test can see of "listed once");
  * a PSD template, a TRI template and method="lsqr": the loop, equal to K calls."""
import numpy as np
import pytest
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_vjp_many import K_BEYOND, KS, SHAPES, ZERO_AT, _draw_of, _point

pytestmark = pytest.mark.gpu

_T: dict = {}


def tangents(K, base_tA, base_tq):
    """(K, B, nnz_aug), (K, B, n + 1) from K_BEYOND - 1 Gaussian draws: draw k at position k, zeros at ZERO_AT and draw 0 again at K - 1 when K >= 3"""
    tA, tq = base_tA[:K].copy(), base_tq[:K].copy()
    if K >= 3:
        tA[ZERO_AT] = 0.0; tq[ZERO_AT] = 0.0
        tA[K - 1] = base_tA[0]; tq[K - 1] = base_tq[0]
    return tA, tq


def _shape(name):
    """the shared point of the shape, Gaussian tangent draws in the value coordinates (the maps are linear: every entry of a value row may move) and the LSQR forward
    derivative of every draw under the tight rule: computed once per shape, shared, not changed"""
    if name in _T:
        return _T[name]
    r = _point(name)
    eng, B = r["eng"], len(r["ok"])
    rng = np.random.default_rng(1000 + r["n"] + B)
    base_tA = rng.standard_normal((K_BEYOND, B, r["tpl"].nnz_aug)); base_tq = rng.standard_normal((K_BEYOND, B, r["n"] + 1))
    lsqr = []
    for k in range(K_BEYOND - 1):
        got = eng.jvp(r["A_bm"], *r["pt"], torch.from_numpy(base_tA[k]).cuda(), torch.from_numpy(base_tq[k]).cuda().t(), path="per_instance", lsqr=TIGHT_LSQR,
                      q_eval=r["q_t"], method="lsqr")
        assert eng.last_jvp_kernel == "ce_jvp_lsqr"
        lsqr.append(tuple(t.cpu().numpy() for t in got))
    t = dict(r=r, B=B, base_tA=base_tA, base_tq=base_tq, lsqr=lsqr, runs={})
    _T[name] = t
    return t


def _run(t, K):
    """jvp_many and its loop for K tangents at the shape's point (once per K): (dx, dy, ds, status, iters) each"""
    if K in t["runs"]:
        return t["runs"][K]
    r = t["r"]; eng = r["eng"]
    tA, tq = tangents(K, t["base_tA"], t["base_tq"])
    tAt, tqt = torch.from_numpy(tA).cuda(), torch.from_numpy(tq).cuda()
    kw = dict(path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    many = eng.jvp_many(r["A_bm"], *r["pt"], tAt, tqt, **kw)
    path, its = eng.last_jvp_many_path, eng.last_lsqr_iters
    loop = eng.jvp_many(r["A_bm"], *r["pt"], tAt, tqt, force_loop=True, **kw)
    assert eng.last_jvp_many_path == "loop"
    its_l = eng.last_lsqr_iters
    torch.cuda.synchronize()
    out = dict(path=path, many=tuple(u.cpu().numpy() for u in many + (its,)), loop=tuple(u.cpu().numpy() for u in loop + (its_l,)), tA=tAt, tq=tqt)
    t["runs"][K] = out
    return out


def _rel(got, want):
    return np.abs(got - want).max(axis=-1) / (1 + np.abs(want).max(axis=-1))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SHAPES)
def test_every_tangent_against_the_loop_of_single_tangent_calls(name, K):
    t = _shape(name)
    o = _run(t, K)
    r = t["r"]
    assert o["path"] == "many"
    assert _lib.lib().ce_jvp_many_variant(r["eng"]._h) == _lib.lib().ce_adjoint_ns_variant(r["eng"]._h) >= 0
    m, l = o["many"], o["loop"]
    assert m[0].shape == (K, t["B"], r["n"]) and m[1].shape == m[2].shape == (K, t["B"], r["tpl"].m) and m[3].shape == m[4].shape == (K, t["B"])
    assert (m[3] == l[3]).all(), (name, K, m[3], l[3])
    assert (m[4] == l[4]).all(), (name, K, m[4], l[4])
    assert ((m[3] & (4 | 8)) == (m[3][:1] & (4 | 8))).all()          # rank deficiency is the matrix's: the same for every tangent
    for i, what in enumerate(("dx", "dy", "ds")):
        e = _rel(m[i], l[i])
        print(f"{name} K={K}: {what} against the loop {e.max():.2e}, flagged {int((m[3][0] != 0).sum())}")
        assert e.max() < 1e-6, (name, K, what, e.max())
    if K >= 3:
        un = m[3][ZERO_AT] == 0
        for i in range(3):
            assert (m[i][ZERO_AT][un] == 0).all()
            assert np.array_equal(m[i][0], m[i][K - 1]), (name, K, i, np.abs(m[i][0] - m[i][K - 1]).max())          # the repeated tangent, first and last: bit for bit


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SHAPES)
def test_every_tangent_against_the_lsqr_forward_derivative(name, K):
    t = _shape(name)
    o = _run(t, K)
    r = t["r"]
    m = o["many"]
    for k in range(K):
        d = _draw_of(K, k)
        if d is None:
            continue
        ref = t["lsqr"][d]
        ref_ok = ref[3] == 0
        assert (r["ok"] & ~ref_ok).mean() <= 0.1, (name, K, k, (r["ok"] & ~ref_ok).mean())
        reg = r["ok"] & (m[3][k] == 0)
        assert reg.mean() >= r["share"], (name, K, k, reg.mean(), np.bincount(m[3][k]))
        cmp_ = reg & ref_ok
        for i, what in enumerate(("dx", "dy", "ds")):
            e = _rel(m[i][k], ref[i])[cmp_]
            print(f"{name} K={K} k={k}: {what} worst {e.max():.2e} median {np.median(e):.2e}, regular {reg.mean():.3f}, reference not converged {int((~ref_ok).sum())}")
            assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, K, k, what, e.max(), np.median(e))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ("small_mixed", "M", "edge_n29"))
def test_transpose_identity_with_vjp_many(name, K):
    """<x-bar_k, dx_j> + <y-bar_k, dy_j> == <dA_k, tA_j> + <dq_k, tq_j> for every pair, to 1e-6 (1 + |lhs| + |rhs|), on the instances both solve directly"""
    from test_gpu_vjp_many import cotangents
    t = _shape(name)
    o = _run(t, K)
    r = t["r"]; eng = r["eng"]
    xb, yb = (torch.from_numpy(a).cuda() for a in cotangents(K, r["base_dx"], r["base_dy"]))
    dA, dq, adj = eng.vjp_many(r["A_bm"], *r["pt"], xb, yb, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"])
    assert eng.last_vjp_many_path == "many"
    dx, dy = (torch.from_numpy(o["many"][i]).cuda() for i in (0, 1))
    lhs = torch.einsum("kbi,jbi->kjb", xb, dx) + torch.einsum("kbi,jbi->kjb", yb, dy)
    rhs = torch.einsum("kbi,jbi->kjb", dA, o["tA"]) + torch.einsum("kbi,jbi->kjb", dq, o["tq"])
    both = torch.from_numpy(r["ok"] & (o["many"][3] == 0).all(axis=0)).cuda() & (adj == 0).all(dim=0)
    assert both.float().mean() >= r["share"]
    lhs, rhs = lhs[:, :, both].cpu().numpy(), rhs[:, :, both].cpu().numpy()
    e = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
    print(f"{name} K={K}: transpose identity {e.max():.2e} on {int(both.sum())} instances")
    assert e.max() < 1e-6 and np.abs(lhs).max() > 1e-3, (name, K, e.max())


@pytest.mark.parametrize("which", ("tq", "tA", "both"))
@pytest.mark.parametrize("name", ("small_mixed", "M"))
def test_batch_shared_tangents_equal_their_expansion_bit_for_bit(name, which):
    t = _shape(name)
    r = t["r"]; eng = r["eng"]
    K, B = 3, t["B"]
    sA = torch.from_numpy(t["base_tA"][:K, 0].copy()).cuda() if which != "tq" else None          # (K, nnz_aug): one row for the batch
    sq = torch.from_numpy(t["base_tq"][:K, 0].copy()).cuda() if which != "tA" else None
    kw = dict(path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    shared = eng.jvp_many(r["A_bm"], *r["pt"], sA, sq, **kw)
    assert eng.last_jvp_many_path == "many"
    its = eng.last_lsqr_iters
    ex = lambda u: None if u is None else u[:, None, :].expand(K, B, u.shape[1]).contiguous()
    full = eng.jvp_many(r["A_bm"], *r["pt"], ex(sA), ex(sq), **kw)
    assert eng.last_jvp_many_path == "many"
    assert all(torch.equal(u, v) for u, v in zip(shared, full)) and torch.equal(its, eng.last_lsqr_iters)
    assert shared[0].abs().max() > 0
    loop = eng.jvp_many(r["A_bm"], *r["pt"], sA, sq, force_loop=True, **kw)          # (the loop expands a shared tangent itself)
    for u, v in zip(shared[:3], loop[:3]):
        e = ((u - v).abs().amax(dim=2) / (1 + v.abs().amax(dim=2))).max().item()
        assert e < 1e-6, (name, which, e)
    assert torch.equal(shared[3], loop[3])


def _degenerate(n, cones, B, seed, mutate, K=3):
    from test_gpu_jvp_direct import _point as direct_point
    r = direct_point(n, cones, B, seed, eps=1e-10, min_solved=0.8, mutate=mutate)
    eng, Bk = r["eng"], int(r["keep"].sum())
    rng = np.random.default_rng(seed + 7)
    tA = torch.from_numpy(rng.standard_normal((K, Bk, r["tpl"].nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((K, Bk, n + 1))).cuda()
    kw = dict(path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    many = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, **kw)
    assert eng.last_jvp_many_path == "many"
    its = eng.last_lsqr_iters
    loop = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, force_loop=True, **kw)
    its_l = eng.last_lsqr_iters
    torch.cuda.synchronize()
    return r, tuple(u.cpu().numpy() for u in many + (its,)), tuple(u.cpu().numpy() for u in loop + (its_l,))


def test_duplicated_equality_rows_are_flagged_for_every_tangent_and_resolved():
    def mutate(A, b):
        deg = np.arange(A.shape[0]) % 2 == 0
        A[deg, 2, :] = A[deg, 0, :]; b[deg, 2] = b[deg, 0]
        return deg
    r, m, l = _degenerate(12, {"z": 4, "l": 8, "q": [5]}, 24, 11, mutate)
    deg = r["extra"][r["keep"]]
    for k in range(m[3].shape[0]):
        assert (m[3][k][deg] == 12).all() and (m[3][k][~deg] == 0).all(), (k, m[3][k])
        assert (m[4][k][deg] > 0).all() and (m[4][k][~deg] == 0).all(), (k, m[4][k])
    assert (m[3] == l[3]).all() and (m[4] == l[4]).all()
    for i, what in enumerate(("dx", "dy", "ds")):
        e = _rel(m[i], l[i])
        print(f"duplicated rows: {what} against the loop {e.max():.2e}")
        assert e.max() < 1e-6, (what, e.max())


def test_lp_vertices_are_flagged_or_solved_for_every_tangent():
    r, m, l = _degenerate(10, {"z": 0, "l": 30, "q": []}, 64, 9, None)
    reg, fl = m[3] == 0, (m[3] & 8) != 0
    print("LP vertices: regular", reg[0].mean(), "flagged", fl[0].mean(), "status counts", np.bincount(m[3][0]))
    assert (reg | fl).all() and reg[0].mean() > 0.5
    assert ((m[3] & 4) != 0).sum() == fl.sum() and (fl == fl[:1]).all() and (m[3][fl] == 12).all()
    assert (m[3] == l[3]).all() and (m[4] == l[4]).all() and (m[4][fl] > 0).all() and (m[4][reg] == 0).all()
    for i, what in enumerate(("dx", "dy", "ds")):
        e = _rel(m[i], l[i])
        print(f"LP vertices: {what} against the loop {e.max():.2e}")
        assert e.max() < 1e-6, (what, e.max())


def _loop_equals_calls(eng, A_bm, pt, q_t, tA, tq, method):
    K = tA.shape[0]
    got = eng.jvp_many(A_bm, *pt, tA, tq, path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t, method=method)
    assert eng.last_jvp_many_path == "loop"
    its = eng.last_lsqr_iters
    assert its.shape == (K, A_bm.shape[0])
    for k in range(K):
        one = eng.jvp(A_bm, *pt, tA[k], tq[k].t(), path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t, method=method)
        assert all(torch.equal(u[k], v) for u, v in zip(got, one)) and torch.equal(its[k], eng.last_lsqr_iters)


@pytest.mark.parametrize("kind", ("psd", "triple", "method_lsqr"))
def test_templates_and_methods_without_the_mode_run_the_loop(kind):
    from test_gpu_jvp_direct import _point as direct_point
    n, cones, B = {"psd": (4, {"z": 1, "s": [3]}, 5), "triple": (6, {"z": 1, "l": 3, "q": [4], "ep": 1}, 8), "method_lsqr": (12, {"z": 2, "l": 6, "q": [4, 5]}, 16)}[kind]
    r = direct_point(n, cones, B, 6 if kind == "psd" else 1, eps=1e-10 if kind == "psd" else 1e-9, min_solved=0.7)
    eng, Bk = r["eng"], int(r["keep"].sum())
    many_v = _lib.lib().ce_jvp_many_variant(eng._h)
    assert (many_v >= 0) == (kind == "method_lsqr")
    rng = np.random.default_rng(4)
    tA = torch.from_numpy(rng.standard_normal((3, Bk, r["tpl"].nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((3, Bk, n + 1))).cuda()
    _loop_equals_calls(eng, r["A_bm"], r["pt"], r["q_t"], tA, tq, "lsqr" if kind == "method_lsqr" else "direct")
    if kind != "method_lsqr":          # the library's own refusal names the reason
        z = torch.zeros((3, Bk, max(n, r["tpl"].m)), dtype=torch.float64, device="cuda"); st = torch.zeros((3, Bk), dtype=torch.int32, device="cuda")
        rc = _lib.lib().ce_jvp_many(eng._h, Bk, 3, r["A_bm"].data_ptr(), eng.nnz_aug, None, 0, 0, *(u.data_ptr() for u in r["pt"]), tA.data_ptr(), tA.stride(0), eng.nnz_aug,
                                    None, 0, 0, z.data_ptr(), z.data_ptr(), None, st.data_ptr(), None, 1e-8, 1e-8, 1e8, 0, None)
        msg = (_lib.lib().ce_last_error() or b"").decode()
        assert rc == -2 and "ce_jvp_many" in msg and "exponential" in msg, (rc, msg)


def test_a_batch_stride_between_one_and_the_row_length_is_refused():
    t = _shape("small_mixed")
    r = t["r"]; eng = r["eng"]
    K, B, L = 2, t["B"], _lib.lib()
    f64 = dict(dtype=torch.float64, device="cuda")
    tA = torch.zeros((K, B, eng.nnz_aug), **f64); tq = torch.zeros((K, B, eng.n + 1), **f64)
    dx, dy = torch.zeros((K, B, eng.n), **f64), torch.zeros((K, B, eng.m), **f64)
    st = torch.full((K, B), -7, dtype=torch.int32, device="cuda")
    A_c = r["A_bm"].contiguous()

    def call(stA_b, stq_b):
        return L.ce_jvp_many(eng._h, B, K, A_c.data_ptr(), eng.nnz_aug, None, 0, 0, *(u.data_ptr() for u in r["pt"]), tA.data_ptr(), tA.stride(0), stA_b,
                             tq.data_ptr(), tq.stride(0), stq_b, dx.data_ptr(), dy.data_ptr(), None, st.data_ptr(), None, 1e-8, 1e-8, 1e8, 0, None)
    for stA_b, stq_b in ((1, eng.n + 1), (eng.nnz_aug - 1, eng.n + 1), (eng.nnz_aug, 1), (eng.nnz_aug, eng.n), (-1, eng.n + 1)):
        assert call(stA_b, stq_b) == -1 and b"batch stride" in L.ce_last_error(), (stA_b, stq_b)
    torch.cuda.synchronize()
    assert (st == -7).all()          # refused before any device call
    assert call(0, 0) == 0 and call(eng.nnz_aug, eng.n + 1) == 0
    torch.cuda.synchronize()
    assert ((st.cpu().numpy() & ~(4 | 8)) == 0).all()


def test_empty_batches_and_no_tangent():
    t = _shape("small_mixed")
    r = t["r"]; eng = r["eng"]
    B, n, m = t["B"], r["n"], r["tpl"].m
    z = torch.zeros((0, B, eng.nnz_aug), dtype=torch.float64, device="cuda")
    dx, dy, ds, st = eng.jvp_many(r["A_bm"], *r["pt"], z, None, path="per_instance", q_eval=r["q_t"])
    assert dx.shape == (0, B, n) and dy.shape == ds.shape == (0, B, m) and st.shape == (0, B) and eng.last_lsqr_iters.shape == (0, B)
    with pytest.raises(ValueError, match="at least one"):
        eng.jvp_many(r["A_bm"], *r["pt"], None, None, path="per_instance", q_eval=r["q_t"])

"""K tangents and K cotangents at one solution of a template with PSD blocks AND exponential / power triples, on one factorisation per instance:
k_backward_ns<..., TRI, MANY, PSD> with and without FWD behind ce_jvp_psd_tri_many / ce_vjp_psd_tri_many, ConeEngine.jvp_many / vjp_many(psd_many=True).  Per
right-hand side the kernel rebuilds both gamma_c = W^T g per triple and gamma = Q^T g per block.

Shapes mix_all, logdet_like and row2_n80 of psd_tri_ns_kit at the oracle's points (eps 1e-10, every instance Solved; the stiff rule flags nothing there), K in
(1, 3, 8); at K >= 3 right-hand side 1 is all zeros and right-hand side 0 is repeated at K - 1 (psd_many_kit.pattern).  Checked against
  * the loop (force_loop=True): K ce_jvp_psd_tri calls in the forward direction, K pivoting ce_vjp calls in the reverse one -- 1e-6 on status-0 instances
    relative to 1 + max |loop|, torch.equal for status (and iteration counts in the forward direction) and for flagged pairs of the forward direction;
  * a batch-shared tangent (stride 0) against its expansion, the repeated right-hand side first and last, bit-identical;
  * the K x K transpose identity between the two many-modes, 1e-6 (1 + |lhs| + |rhs|);
  * the plan's edges: ce_jvp_psd_tri and both many-modes (K = 2, B = 4) at n in (28, 29, 60, 61, 108) against ce_jvp_lsqr / the loop; n = 109 is refused."""
import numpy as np
import pytest
import torch

import psd_many_kit as M
import psd_tri_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_jvp import _engine, _tangents

pytestmark = pytest.mark.gpu
KS = (1, 3, 8)
KW = dict(path="per_instance", lsqr=TIGHT_LSQR, method="direct")
_POINTS: dict = {}
EDGE_CONES = {"z": 2, "l": 4, "s": [3], "ep": 1}
EDGE_ROWS = {28: 0, 29: 1, 60: 1, 61: 2, 108: 2}          # n -> row of CE_NS_VARIANTS (4 ceil(n / 4) + 1 <= 32 / 64 / 112 columns)
_REACHED: dict = {}


def _make(n, cones, A, b, c, ref, seed, n_draws):
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    B = A.shape[0]
    rng = np.random.default_rng(seed + 1)
    base_dx = rng.standard_normal((n_draws,) + ref["x"].shape); base_dy = rng.standard_normal((n_draws,) + ref["y"].shape)
    base_tA = np.zeros((n_draws, B, tpl.nnz_aug)); base_tq = np.zeros((n_draws, B, n + 1))
    for k in range(n_draws):
        _, tA_bm, tq = _tangents(tpl, B, seed=seed + 100 + k)
        base_tA[k] = tA_bm.cpu().numpy(); base_tq[k] = tq.cpu().numpy().T
    return dict(n=n, cones=cones, tpl=tpl, A=A, ref=ref, eng=_engine(tpl), A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(), q_t=torch.from_numpy(q_eval).cuda(),
                pt=tuple(torch.from_numpy(ref[k]).cuda() for k in "xys"), base_dx=base_dx, base_dy=base_dy, base_tA=base_tA, base_tq=base_tq, runs={})


def _point(name):
    """problem, oracle point, engine, device tensors and the Gaussian draws of both directions: once per shape, shared, not changed"""
    if name not in _POINTS:
        n, cones, A, b, c, ref = K.problem(name)
        assert (ref["status"] == 1).all(), ref["status"]
        _POINTS[name] = _make(n, cones, A, b, c, ref, K.SHAPES[name][3], max(KS))
        assert _lib.lib().ce_jvp_psd_tri_many_variant(_POINTS[name]["eng"]._h) == _lib.lib().ce_vjp_psd_tri_many_variant(_POINTS[name]["eng"]._h) == K.PLAN[name][0]
    return _POINTS[name]


def _run_jvp(r, Kc, loop=False):
    key = ("jvp", Kc, loop)
    if key not in r["runs"]:
        eng = r["eng"]
        tA, tq = (torch.from_numpy(a).cuda() for a in M.pattern(Kc, r["base_tA"], r["base_tq"]))
        got = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], psd_many=True, force_loop=loop, **KW)
        r["runs"][key] = dict(path=eng.last_jvp_many_path, kernel=eng.last_jvp_kernel, out=tuple(got) + (eng.last_lsqr_iters,), tA=tA, tq=tq)
        torch.cuda.synchronize()
    return r["runs"][key]


def _run_vjp(r, Kc, loop=False):
    key = ("vjp", Kc, loop)
    if key not in r["runs"]:
        eng = r["eng"]
        dx, dy = (torch.from_numpy(a).cuda() for a in M.pattern(Kc, r["base_dx"], r["base_dy"]))
        got = eng.vjp_many(r["A_bm"], *r["pt"], dx, dy, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], psd_many=True, force_loop=loop)
        r["runs"][key] = dict(path=eng.last_vjp_many_path, kernel=eng.last_vjp_kernel, out=tuple(got), dx=dx, dy=dy)
        torch.cuda.synchronize()
    return r["runs"][key]


def _check_jvp_against_loop(r, Kc, what, share=M.MIN_SHARE):
    o, l = _run_jvp(r, Kc), _run_jvp(r, Kc, loop=True)
    assert (o["path"], o["kernel"]) == ("many", "ce_jvp_psd_tri_many") and (l["path"], l["kernel"]) == ("loop", "ce_jvp_psd_tri"), (o["kernel"], l["kernel"])
    m, lo = o["out"], l["out"]
    assert torch.equal(m[3], lo[3]) and torch.equal(m[4], lo[4]), (what, Kc, m[3], lo[3], m[4], lo[4])
    st = m[3]
    assert ((st & 12) == (st[:1] & 12)).all()          # flags are the matrix's: equal across k
    reg = st == 0
    assert (reg.double().mean(dim=1) >= share).all()
    for i, nm in enumerate(("dx", "dy", "ds")):
        e = ((m[i] - lo[i]).abs().amax(dim=2) / (1 + lo[i].abs().amax(dim=2)))[reg]
        emax = e.max().item() if e.numel() else 0.0
        print(f"{what} K={Kc}: {nm} against the loop {emax:.2e} on status 0; flagged {int((st[0] != 0).sum())} of {st.shape[1]}")
        assert emax < 1e-6, (what, Kc, nm, emax)
        assert torch.equal(m[i][~reg], lo[i][~reg]), (what, Kc, nm)          # a flagged pair is the same from-scratch LSQR solve in both routes
    assert m[0].abs().max() > 0
    if Kc >= 3:
        un = st[M.ZERO_AT] == 0
        for i in range(3):
            assert (m[i][M.ZERO_AT][un] == 0).all()
            assert torch.equal(m[i][0], m[i][Kc - 1]), (what, Kc, i)          # the repeated tangent, first and last: bit for bit


def _check_vjp_against_loop(r, Kc, what, share=M.MIN_SHARE):
    o, l = _run_vjp(r, Kc), _run_vjp(r, Kc, loop=True)
    assert (o["path"], o["kernel"]) == ("many", "ce_vjp_psd_tri_many") and (l["path"], l["kernel"]) == ("loop", None), (o["kernel"], l["kernel"])
    (dA, dq, adj), (lA, lq, ladj) = o["out"], l["out"]
    assert ((adj & 12) == (adj[:1] & 12)).all()          # flags are the matrix's: equal across k
    reg = (adj == 0) & (ladj == 0)          # (the pivoting kernel need not flag the same instances)
    assert (reg.double().mean(dim=1) >= share).all(), (adj, ladj)
    for got, want, nm in ((dA, lA, "dA"), (dq, lq, "dq")):
        e = ((got - want).abs().amax(dim=2) / (1 + want.abs().amax(dim=2)))[reg]
        emax = e.max().item() if e.numel() else 0.0
        print(f"{what} K={Kc}: {nm} against the loop of pivoting ce_vjp calls {emax:.2e} on status 0; flagged {int((adj[0] != 0).sum())} of {adj.shape[1]}")
        assert emax < 1e-6, (what, Kc, nm, emax)
    fl = adj[0] != 0
    if fl.any():          # a flagged instance: 4 | 8 for every k, and the answer of the LSQR adjoint (the same kernel under the same rule) to 1e-6
        assert (adj[:, fl] == 12).all(), adj
        for k in range(Kc):
            wA, wq, wadj = r["eng"].vjp(r["A_bm"], *r["pt"], o["dx"][k], o["dy"][k], path="per_instance_lsqr", lsqr=TIGHT_LSQR, q_eval=r["q_t"])
            for got, want, nm in ((dA[k], wA.t(), "dA"), (dq[k], wq.t(), "dq")):
                e = (got[fl] - want[fl]).abs().max().item() / (1 + want[fl].abs().max().item())
                print(f"{what} K={Kc} k={k}: {nm} re-solved against the LSQR adjoint {e:.2e}")
                assert e < 1e-6, (what, Kc, k, nm, e)
    assert dA.abs().max() > 0
    if Kc >= 3:
        un = adj[M.ZERO_AT] == 0
        assert (dA[M.ZERO_AT][un] == 0).all() and (dq[M.ZERO_AT][un] == 0).all()
        assert torch.equal(dA[0], dA[Kc - 1]) and torch.equal(dq[0], dq[Kc - 1]) and torch.equal(adj[0], adj[Kc - 1]), (what, Kc)          # the repeat: bit for bit


@pytest.mark.parametrize("Kc", KS)
@pytest.mark.parametrize("name", ["mix_all", "logdet_like", "row2_n80"])
def test_every_tangent_against_the_loop_of_single_tangent_calls(name, Kc):
    """fails on a tree without the mode: the loop's kernel is ce_jvp_lsqr there and no call is ce_jvp_psd_tri_many"""
    _check_jvp_against_loop(_point(name), Kc, name)


@pytest.mark.parametrize("Kc", KS)
@pytest.mark.parametrize("name", ["mix_all", "logdet_like", "row2_n80"])
def test_every_cotangent_against_the_loop_of_pivoting_calls(name, Kc):
    _check_vjp_against_loop(_point(name), Kc, name)


@pytest.mark.parametrize("which", ("tq", "tA", "both"))
def test_batch_shared_tangents_equal_their_expansion_bit_for_bit(which):
    r = _point("mix_all")
    eng, Kc, B = r["eng"], 3, r["A"].shape[0]
    sA = torch.from_numpy(r["base_tA"][:Kc, 0].copy()).cuda() if which != "tq" else None          # (K, nnz_aug): one row for the batch
    sq = torch.from_numpy(r["base_tq"][:Kc, 0].copy()).cuda() if which != "tA" else None
    shared = eng.jvp_many(r["A_bm"], *r["pt"], sA, sq, q_eval=r["q_t"], psd_many=True, **KW)
    assert eng.last_jvp_kernel == "ce_jvp_psd_tri_many"
    its = eng.last_lsqr_iters
    ex = lambda u: None if u is None else u[:, None, :].expand(Kc, B, u.shape[1]).contiguous()          # noqa: E731
    full = eng.jvp_many(r["A_bm"], *r["pt"], ex(sA), ex(sq), q_eval=r["q_t"], psd_many=True, **KW)
    assert eng.last_jvp_kernel == "ce_jvp_psd_tri_many"
    assert all(torch.equal(u, v) for u, v in zip(shared, full)) and torch.equal(its, eng.last_lsqr_iters)
    assert shared[0].abs().max() > 0


@pytest.mark.parametrize("name", ["mix_all", "logdet_like"])
def test_transpose_identity_between_the_two_many_modes(name):
    """<x-bar_k, dx_j> + <y-bar_k, dy_j> == <dA_k, tA_j> + <dq_k, tq_j> for every pair, to 1e-6 (1 + |lhs| + |rhs|), where both modes report status 0"""
    r = _point(name)
    Kc = 3
    o, v = _run_jvp(r, Kc), _run_vjp(r, Kc)
    assert o["kernel"] == "ce_jvp_psd_tri_many" and v["kernel"] == "ce_vjp_psd_tri_many"
    dA, dq, adj = v["out"]
    xb, yb = v["dx"], v["dy"]
    dx, dy, _, st, _ = o["out"]
    lhs = torch.einsum("kbi,jbi->kjb", xb, dx) + torch.einsum("kbi,jbi->kjb", yb, dy)
    rhs = torch.einsum("kbi,jbi->kjb", dA, o["tA"]) + torch.einsum("kbi,jbi->kjb", dq, o["tq"])
    both = (st == 0).all(dim=0) & (adj == 0).all(dim=0)
    assert both.double().mean().item() >= M.MIN_SHARE
    lhs, rhs = lhs[:, :, both].cpu().numpy(), rhs[:, :, both].cpu().numpy()
    e = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
    print(f"{name}: K x K transpose identity {e.max():.2e} on {int(both.sum())} instances")
    assert e.max() < 1e-6 and np.abs(lhs).max() > 1e-3, (name, e.max())


def _edge(n):
    key = ("edge", n)
    if key not in _POINTS:
        from oracle import oracle
        A, b, c = P.generate(n, EDGE_CONES, 4, seed=n)
        ref = oracle.solve_batch(A, b, c, EDGE_CONES, eps=1e-10, max_iters=200000)
        assert (ref["status"] == 1).all(), (n, ref["status"])
        _POINTS[key] = _make(n, EDGE_CONES, A, b, c, ref, n, 2)
    return _POINTS[key]


@pytest.mark.parametrize("n", list(EDGE_ROWS))
def test_the_three_modes_at_the_edges_of_the_plan(n):
    """ce_jvp_psd_tri against ce_jvp_lsqr (1e-5 worst on status-0 instances under the tight rule, 1e-6 on re-solved ones), both many-modes (K = 2, B = 4) against
    the loop.  With these cones m = 15 < n: checked on the CPU with the oracle, every instance is Solved but its x is not unique, so the elimination finds the
    reduced Hessian singular and hands every instance to the re-solve (status 4 | 8) -- the rows' kernels run at their largest and smallest n all the same, and what
    is compared is the re-solved answer (LSQR's minimum-norm one in every route), not a share of directly solved instances.  The directly solved half -- the same
    edges at planted KKT points with m > n, every instance status 0, against dense references -- is tests/test_gpu_psd_mode_edges.py."""
    r = _edge(n)
    eng, L = r["eng"], _lib.lib()
    assert L.ce_psd_tri_ns_variant(eng._h) == L.ce_vjp_psd_tri_many_variant(eng._h) == L.ce_jvp_psd_tri_many_variant(eng._h) == EDGE_ROWS[n] == K.host_plan(n, EDGE_CONES)["psd_tri_ns_variant"]
    tA, tq = torch.from_numpy(r["base_tA"][0]).cuda(), torch.from_numpy(r["base_tq"][0].T.copy()).cuda()
    d = eng.jvp(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], psd_ns=True, **KW)
    assert eng.last_jvp_kernel == "ce_jvp_psd_tri"
    its = eng.last_lsqr_iters
    l = eng.jvp(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], path="per_instance", lsqr=TIGHT_LSQR, method="lsqr")
    assert eng.last_jvp_kernel == "ce_jvp_lsqr"
    reg, fl = (d[3] == 0) & (l[3] == 0), (d[3] == 12) & (l[3] == 0)
    print(f"n={n}: status {d[3].tolist()} iterations {its.tolist()}")
    assert (reg | fl).all() and (its[reg] == 0).all() and (its[fl] > 0).all(), (d[3], l[3], its)
    for i, nm in enumerate(("dx", "dy", "ds")):
        e = (d[i] - l[i]).abs().amax(dim=1) / (1 + l[i].abs().amax(dim=1))
        print(f"n={n}: {nm} against ce_jvp_lsqr {e.max().item():.2e}")
        assert (e[reg] < 1e-5).all() and (e[fl] < 1e-6).all(), (n, nm, e)
    _check_jvp_against_loop(r, 2, f"n={n}", share=0.0)
    _check_vjp_against_loop(r, 2, f"n={n}", share=0.0)
    _REACHED[n] = EDGE_ROWS[n]


def test_every_row_is_reached_and_n_109_is_refused():
    import plan_kit as pk
    rows = [r[0] for r in pk.variant_rows("CE_NS_VARIANTS")]
    assert rows == [0, 1, 2], rows
    for n in EDGE_ROWS:
        if n not in _REACHED:
            test_the_three_modes_at_the_edges_of_the_plan(n)
    assert {_REACHED[n] for n in EDGE_ROWS} == set(rows)
    eng = _engine(P.dense_template(109, EDGE_CONES))
    L = _lib.lib()
    assert L.ce_psd_tri_ns_variant(eng._h) == -1 == L.ce_vjp_psd_tri_many_variant(eng._h) == L.ce_jvp_psd_tri_many_variant(eng._h) and L.ce_psd_tri_ns_lds(eng._h) == 0
    assert K.host_plan(109, EDGE_CONES)["psd_tri_ns_variant"] == -1
    buf = torch.zeros(8192, dtype=torch.float64, device="cuda"); p = buf.data_ptr()
    assert L.ce_jvp_psd_tri(eng._h, 1, p, eng.nnz_aug, None, 0, 0, p, p, p, None, 0, None, 0, 0, p, p, None, p, None, 1e-8, 1e-8, 1e8, 0, None) == -2
    assert "ce_jvp_psd_tri:" in (L.ce_last_error() or b"").decode() and "n > 108" in (L.ce_last_error() or b"").decode()


def test_without_the_flag_both_directions_run_their_loops_as_today():
    r = _point("mix_all")
    eng, Kc = r["eng"], 2
    tA, tq = (torch.from_numpy(a).cuda() for a in M.pattern(Kc, r["base_tA"], r["base_tq"]))
    eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], **KW)
    assert (eng.last_jvp_many_path, eng.last_jvp_kernel) == ("loop", "ce_jvp_lsqr")
    eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], tri_many=True, **KW)          # tri_many stays inert beside a PSD block
    assert (eng.last_jvp_many_path, eng.last_jvp_kernel) == ("loop", "ce_jvp_lsqr")
    dx, dy = (torch.from_numpy(a).cuda() for a in M.pattern(Kc, r["base_dx"], r["base_dy"]))
    for kw in ({}, {"tri_many": True}):
        eng.vjp_many(r["A_bm"], *r["pt"], dx, dy, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], **kw)
        assert (eng.last_vjp_many_path, eng.last_vjp_kernel) == ("loop", None)

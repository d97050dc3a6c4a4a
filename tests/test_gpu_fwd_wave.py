"""k_fwd_wave (ce_solve_wave): the forward solve of a small template, one instance per wave, against the CPU oracle and against ce_solve on the same inputs.
The conditions are run_parity's own (tests/test_gpu_parity.py) and hold on EVERY instance: status equal, x / y / s within max(1e-6, 20 eps) (1 + |.|_inf), iteration
counts within 25 (one check interval).  Shapes: every instantiation of csrc/ce_variants_wave.h at and inside its bounds, one cone over all rows, cones of 1 and 2 rows.
Beside them: known answers and certificates, every setting the kernel honours, sparsity patterns, warm starts, batch edges, purity under permutation, the refusals
and what the call leaves on the handle."""
import ctypes as C

import numpy as np
import pytest
import torch

import kit
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P

pytestmark = pytest.mark.gpu

SHAPES = [(2, dict(z=0, l=3, q=[])),
          (3, dict(z=1, l=2, q=[1, 3])),
          (8, dict(z=2, l=6, q=[3, 5])),
          (16, dict(z=2, l=10, q=[4, 16])),
          (31, dict(z=3, l=17, q=[2, 7, 34])),
          (32, dict(z=4, l=20, q=[8, 32])),
          (32, dict(z=0, l=0, q=[64]))]
B0, SEED, EPS, MAXIT = 67, 5, 1e-8, 20000
MID = SHAPES[2]


def _engine(tpl, p_structure=None):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    return ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0), p_structure=p_structure)


def _inputs(eng, tpl, A, b, c, batch_minor=True):
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    A_t = torch.from_numpy(A_eval).cuda()
    if not batch_minor:
        A_t = A_t.t().contiguous().t()
    return eng.to_batch_major(A_t), torch.from_numpy(q_eval).cuda()


def _solve(eng, A_bm, q_t, wave, warm=None, **args):
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    args.setdefault("acceleration_lookback", 0)      # the oracle's default: plain iteration
    args.setdefault("eps", EPS); args.setdefault("max_iters", MAXIT)
    x, y, s, iters, status, resid = eng.solve(A_bm, q_t, make_settings(args), warm=warm, wave=wave)
    torch.cuda.synchronize()
    assert eng.last_path == "per_instance" and eng.last_forward_kernel == ("k_fwd_wave" if wave else None)
    return dict(x=x.cpu().numpy(), y=y.cpu().numpy(), s=s.cpu().numpy(), iters=iters.cpu().numpy(), status=status.cpu().numpy(), resid=resid.cpu().numpy(), t=(x, y, s, iters, status))


def _same(got, want, eps=EPS, what=""):
    """run_parity's conditions, on every instance"""
    assert (got["status"] == want["status"]).all(), (what, got["status"], want["status"])
    tol = max(1e-6, 20 * eps)
    for k in ("x", "y", "s"):
        err = np.abs(got[k] - want[k]).max(axis=1) / (1 + np.abs(want[k]).max(axis=1))
        print(f"{what} {k}: max err {err.max():.3e} (tol {tol:.1e})")
        assert err.max() < tol, (what, k, err.max())
    d = np.abs(got["iters"].astype(int) - want["iters"].astype(int))
    print(f"{what} iters: max diff {d.max()}, range {want['iters'].min()}..{want['iters'].max()}")
    assert d.max() <= 25, (what, got["iters"], want["iters"])


_CACHE = {}


def _case(n, cones, pattern=None):
    key = (n, repr(cones), None if pattern is None else pattern.tobytes())
    if key not in _CACHE:
        tpl = P.dense_template(n, cones, pattern=pattern)
        A, b, c = P.generate(n, cones, B0, seed=SEED, pattern=pattern)
        eng = _engine(tpl)
        _CACHE[key] = (tpl, A, b, c, eng) + _inputs(eng, tpl, A, b, c)
    return _CACHE[key]


@pytest.mark.parametrize("lookback", [0, 1])
@pytest.mark.parametrize("n,cones", SHAPES, ids=[f"n{n}m{P.cone_rows(c)}" for n, c in SHAPES])
def test_parity_with_the_oracle_and_with_ce_solve(n, cones, lookback):
    from oracle import oracle
    tpl, A, b, c, eng, A_bm, q_t = _case(n, cones)
    assert eng.wave_plan()[0] >= 0 and eng.wave_plan()[1] > 0
    ref = oracle.solve_batch(A, b, c, cones, eps=EPS, max_iters=MAXIT, acceleration_lookback=lookback)
    assert (ref["status"] == 1).all()
    got = _solve(eng, A_bm, q_t, True, acceleration_lookback=lookback)
    _same(got, ref, what=f"wave vs oracle n={n} aa={lookback}")
    _same(got, _solve(eng, A_bm, q_t, False, acceleration_lookback=lookback), what=f"wave vs ce_solve n={n} aa={lookback}")
    if n == 8:      # the early-exit case: short and long instances side by side in one launch
        assert ref["iters"].min() <= 100 and ref["iters"].max() >= 1000, ref["iters"]


def test_known_answers():
    for (A, b, c, cones, xstar), nx in ((kit.relu_proj(np.array([1.5, -0.5, 0.25, -2.0])), 4), (kit.box_qp(np.array([2.0, 0.5, -1.0])), 3),
                                        (kit.simplex_lp(np.array([1.0, 2.0, 0.5])), 3), (kit.soc_lin(np.array([1.0, 0.5, -0.5]), 2.0), 3)):
        tpl = P.dense_template(A.shape[1], cones)
        eng = _engine(tpl)
        got = _solve(eng, *_inputs(eng, tpl, A[None], b[None], c[None]), True, eps=1e-10)
        assert got["status"][0] == 1
        np.testing.assert_allclose(got["x"][0, :nx], xstar, atol=1e-5)


def test_certificates_and_their_nan_conventions():
    for builder, want in ((kit.infeasible, -2), (kit.unbounded, -1)):
        A, b, c, cones = builder()
        tpl = P.dense_template(A.shape[1], cones)
        eng = _engine(tpl)
        A_bm, q_t = _inputs(eng, tpl, A[None], b[None], c[None])
        got, base = _solve(eng, A_bm, q_t, True, eps=1e-6), _solve(eng, A_bm, q_t, False, eps=1e-6)
        assert got["status"][0] == want == base["status"][0]
        for k in ("x", "y", "s"):
            assert (np.isnan(got[k]) == np.isnan(base[k])).all(), (want, k)
            ok = ~np.isnan(base[k])
            np.testing.assert_allclose(got[k][ok], base[k][ok], rtol=1e-5, atol=1e-7)
        assert np.isnan(got["x"]).all() == (want == -2) and np.isnan(got["y"]).all() == (want == -1)


def test_out_of_iterations_gives_the_oracles_inaccurate_status():
    from oracle import oracle
    n, cones = MID
    tpl, A, b, c, eng, A_bm, q_t = _case(n, cones)
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-12, max_iters=30)
    got = _solve(eng, A_bm, q_t, True, eps=1e-12, max_iters=30)
    assert (ref["status"] != 1).all()
    assert (got["status"] == ref["status"]).all() and (got["iters"] == 30).all(), (got["status"], ref["status"])


@pytest.mark.parametrize("setting", [dict(normalize=0), dict(adaptive_scale=0), dict(alpha=1.0), dict(scale=1.0), dict(acceleration_interval=5, acceleration_lookback=1)],
                         ids=lambda d: "-".join(d))
def test_settings_against_the_oracle(setting):
    from oracle import oracle
    n, cones = MID
    tpl, A, b, c, eng, A_bm, q_t = _case(n, cones)
    ref = oracle.solve_batch(A, b, c, cones, eps=EPS, max_iters=MAXIT, **setting)
    _same(_solve(eng, A_bm, q_t, True, **setting), ref, what=f"wave vs oracle {setting}")


def _random_pattern(m, n, seed):
    rng = np.random.default_rng(seed)
    pattern = rng.random((m, n)) < 0.6
    pattern[np.arange(m), rng.integers(0, n, m)] = True
    pattern[rng.integers(0, m, n), np.arange(n)] = True
    return pattern


def test_sparse_pattern():
    from oracle import oracle
    cones = dict(z=2, l=5, q=[3, 1, 6]); n = 12
    pattern = _random_pattern(P.cone_rows(cones), n, 7)
    tpl, A, b, c, eng, A_bm, q_t = _case(n, cones, pattern)
    ref = oracle.solve_batch(A, b, c, cones, eps=EPS, max_iters=MAXIT)
    _same(_solve(eng, A_bm, q_t, True), ref, what="sparse pattern")


def test_empty_column_and_rows_without_a_b_entry():
    """relu_proj: its nonnegative rows have b = 0 (left out of the structure); a variable that appears in no constraint and has zero cost is an empty column"""
    t = np.array([1.5, -0.5, 0.25, -2.0])
    A, b, c, cones, xstar = kit.relu_proj(t)
    A = np.concatenate([A, np.zeros((A.shape[0], 1))], axis=1); c = np.concatenate([c, [0.0]])      # the empty column
    pattern = A != 0
    assert not pattern[:, -1].any() and (b == 0).any()
    tpl = P.dense_template(A.shape[1], cones, pattern=pattern, b_pattern=b != 0)
    eng = _engine(tpl)
    A_bm, q_t = _inputs(eng, tpl, A[None], b[None], c[None])
    got, base = _solve(eng, A_bm, q_t, True, eps=1e-10), _solve(eng, A_bm, q_t, False, eps=1e-10)
    assert got["status"][0] == 1 == base["status"][0]
    np.testing.assert_allclose(got["x"][0, :4], xstar, atol=1e-5)
    np.testing.assert_allclose(got["x"][0], base["x"][0], atol=1e-5)


def test_batch_minor_values_give_the_same_bits():
    n, cones = MID
    tpl, A, b, c, eng, A_bm, q_t = _case(n, cones)
    L = _lib.lib()
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    st = make_settings(dict(eps=EPS, max_iters=MAXIT, acceleration_lookback=0))
    A_minor = A_bm.t().contiguous()          # (nnz_aug, B) contiguous: sA_k = B, sA_b = 1
    outs = []
    for ptr, sk, sb in ((A_bm.data_ptr(), 1, tpl.nnz_aug), (A_minor.data_ptr(), B0, 1)):
        x = torch.empty((B0, tpl.n), dtype=torch.float64, device="cuda"); y = torch.empty((B0, tpl.m), dtype=torch.float64, device="cuda"); s = torch.empty_like(y)
        it = torch.empty((B0,), dtype=torch.int32, device="cuda"); stt = torch.empty_like(it)
        rc = L.ce_solve_wave(eng._h, B0, ptr, sk, sb, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), C.byref(st), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                             it.data_ptr(), stt.data_ptr(), None, eng._stream())
        assert rc == 0, L.ce_last_error()
        torch.cuda.synchronize()
        outs.append((x, y, s, it, stt))
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)


def test_warm_start_follows_the_oracles_and_a_nan_point_starts_cold():
    from oracle import oracle
    n, cones = MID
    tpl, A, b, c, eng, A_bm, q_t = _case(n, cones)
    r0 = oracle.solve_batch(A, b, c, cones, eps=1e-4, max_iters=MAXIT)
    warm = [r0["x"].copy(), r0["y"].copy(), r0["s"].copy()]
    warm[1][5, 0] = np.nan                                 # instance 5, and only that one, starts cold
    rw = oracle.solve_batch(A, b, c, cones, eps=EPS, max_iters=MAXIT, warm=warm)
    rc = oracle.solve_batch(A, b, c, cones, eps=EPS, max_iters=MAXIT)
    assert rw["iters"][5] == rc["iters"][5]
    wt = tuple(torch.from_numpy(w).cuda() for w in warm)
    got = _solve(eng, A_bm, q_t, True, warm=wt)
    _same(got, rw, what="warm start")
    cold = _solve(eng, A_bm, q_t, True)
    assert got["iters"][5] == cold["iters"][5] and np.array_equal(got["x"][5], cold["x"][5])
    others = np.arange(B0) != 5
    assert (got["iters"][others] != cold["iters"][others]).any()


@pytest.mark.parametrize("lookback", [0, 1])
def test_batch_edges_and_purity_under_permutation(lookback):
    """an instance's bits depend neither on its position nor on its neighbours: every batch size gives the rows of the full batch, a permuted batch the permuted rows"""
    n, cones = MID
    tpl, A, b, c, eng, A_bm, q_t = _case(n, cones)
    full = _solve(eng, A_bm, q_t, True, acceleration_lookback=lookback)["t"]
    for B in (1, 2, 63, 64, 65, 67):
        part = _solve(eng, A_bm[:B].contiguous(), q_t[:, :B].contiguous(), True, acceleration_lookback=lookback)["t"]
        for a_, f_ in zip(part, full):
            assert torch.equal(a_, f_[:B]), B
    perm = torch.from_numpy(np.random.default_rng(3).permutation(B0)).cuda()
    got = _solve(eng, A_bm[perm].contiguous(), q_t[:, perm].contiguous(), True, acceleration_lookback=lookback)["t"]
    for a_, f_ in zip(got, full):
        assert torch.equal(a_, f_[perm])


def test_refusals_name_the_reason_and_write_nothing():
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    L = _lib.lib()
    p_idx, p_ptr = np.arange(4, dtype=np.int32), np.arange(5, dtype=np.int32)
    cases = [(33, dict(z=0, l=40, q=[]), None, "n > 32"), (4, dict(z=0, l=3, q=[], s=[2]), None, "PSD"), (4, dict(z=0, l=3, q=[], ep=1), None, "exponential"),
             (4, dict(z=0, l=6, q=[]), (p_idx, p_ptr), "P structure")]
    for n, cones, pstruct, word in cases:
        tpl = P.dense_template(n, cones)
        eng = _engine(tpl, p_structure=pstruct)
        assert eng.wave_plan() == (-1, 0)
        B = 3
        A = torch.ones((B, tpl.nnz_aug), dtype=torch.float64, device="cuda"); q = torch.ones((n + 1, B), dtype=torch.float64, device="cuda")
        x = torch.full((B, n), 7.0, dtype=torch.float64, device="cuda"); y = torch.full((B, tpl.m), 7.0, dtype=torch.float64, device="cuda"); s = y.clone()
        it = torch.full((B,), 7, dtype=torch.int32, device="cuda"); stt = it.clone()
        st = make_settings({})
        rc = L.ce_solve_wave(eng._h, B, A.data_ptr(), 1, tpl.nnz_aug, q.data_ptr(), q.stride(0), q.stride(1), C.byref(st), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                             it.data_ptr(), stt.data_ptr(), None, eng._stream())
        assert rc == -2 and word in L.ce_last_error().decode(), (rc, L.ce_last_error())
        torch.cuda.synchronize()
        assert (x == 7).all() and (y == 7).all() and (s == 7).all() and (it == 7).all() and (stt == 7).all()
        with pytest.raises(Exception, match="ce_solve_wave"):
            eng.solve(A, q, make_settings({}), wave=True)


def test_retention_for_the_adjoint_and_the_dispatch_history_left_alone():
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    L = _lib.lib()
    n, cones = MID
    tpl, A, b, c, eng, A_bm, q_t = _case(n, cones)
    st = lambda: make_settings(dict(eps=1e-4, max_iters=MAXIT, acceleration_lookback=10))
    # ce_vjp with A_vals == NULL after ce_solve_wave reads the retained rows
    x, y, s, iters, status = _solve(eng, A_bm, q_t, True)["t"]
    rng = np.random.default_rng(11)
    dx = torch.from_numpy(rng.standard_normal((B0, tpl.n))).cuda(); dy = torch.from_numpy(rng.standard_normal((B0, tpl.m))).cuda()
    outs = []
    for ptr in (A_bm.data_ptr(), None):
        dA = torch.empty((B0, tpl.nnz_aug), dtype=torch.float64, device="cuda"); dq = torch.empty((tpl.n + 1, B0), dtype=torch.float64, device="cuda")
        adj = torch.empty((B0,), dtype=torch.int32, device="cuda")
        rc = L.ce_vjp(eng._h, B0, ptr, 1, tpl.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(), dx.data_ptr(), dy.data_ptr(),
                      dA.data_ptr(), 1, tpl.nnz_aug, dq.data_ptr(), B0, 1, adj.data_ptr(), eng._stream())
        assert rc == 0, L.ce_last_error()
        torch.cuda.synchronize()
        outs.append((dA, dq, adj))
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)
    # an ordinary solve with the dispatch history on gives its bits with or without a wave solve in between
    eng.set_dispatch_history(False)
    ref = [t.clone() for t in eng.solve(A_bm, q_t, st())]
    eng.set_dispatch_history(True)
    try:
        for _ in range(3):
            got = [t.clone() for t in eng.solve(A_bm, q_t, st())]
            for a_, b_ in zip(got, ref):
                assert torch.equal(a_, b_)
            eng.solve(A_bm, q_t, st(), wave=True)
        got = [t.clone() for t in eng.solve(A_bm, q_t, st())]
        for a_, b_ in zip(got, ref):
            assert torch.equal(a_, b_)
    finally:
        eng.set_dispatch_history(False)

"""k_fwd_wave_qp (ce_solve_qp_wave): the forward solve of a small quadratic program, one instance per wave, against the CPU oracle's QP embedding
(oracle.solve_batch(..., P=...), float64, the same algorithm) and against ce_solve_qp on the same inputs.  The conditions are test_gpu_fwd_wave.py's and hold on
EVERY instance: status equal, x / y / s within max(1e-6, 20 eps) (1 + |.|_inf), iteration counts within 25 (one check interval).  Shapes: the smallest, every row
of csrc/ce_variants_fwd_wave_qp.h at its bounds, the first shape of the second row, a mixed one with zero rows and cones of 1 and 5 rows.  P: positive definite,
rank n / 2, diagonal-only and full symmetric structures.  Beside them: warm start, batch-minor values, batch edges and purity under permutation, an indefinite P,
the refusals and what the call leaves on the handle."""
import ctypes as C

import numpy as np
import pytest
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from qp_ns_kit import device_values, full_structure, qp_engine, quad_matrices
from test_gpu_fwd_wave import _same
from test_quad_objective import _upper_structure

pytestmark = pytest.mark.gpu

SHAPES = [(2, dict(z=0, l=3, q=[])),
          (8, dict(z=2, l=6, q=[3, 5])),
          (9, dict(z=1, l=8, q=[3, 5])),
          (16, dict(z=2, l=10, q=[4, 16])),
          (32, dict(z=4, l=20, q=[8, 32])),
          (12, dict(z=2, l=6, q=[1, 5]))]
MIXED, MID = SHAPES[5], SHAPES[1]
B0, SEED, MAXIT = 8, 5, 20000


def _diag_structure(n):
    return np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32), (n, n)


# name -> (structure of n, rank of the draw or None: full with 1/2 I added)
VARIANTS = {"pd_upper": (_upper_structure, None), "rank_half_upper": (_upper_structure, "half"), "diagonal": (_diag_structure, None), "full_symmetric": (full_structure, None)}
_CACHE = {}


def _case(n, cones, variant="pd_upper", B=B0):
    key = (n, repr(cones), variant, B)
    if key not in _CACHE:
        make, rank = VARIANTS[variant]
        struct = make(n)
        tpl = P.dense_template(n, cones)
        A, b, c = P.generate(n, cones, B, seed=SEED)
        Pm = quad_matrices(n, B, SEED, n // 2 if rank else None)
        if variant == "diagonal":
            Pm = Pm * np.eye(n)
        eng = qp_engine(tpl, struct)
        _CACHE[key] = (tpl, A, b, c, Pm, eng) + device_values(tpl, A, b, c, Pm, struct)
    return _CACHE[key]


def _solve(eng, A_bm, q_t, P_bm, wave, warm=None, **args):
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    args.setdefault("acceleration_lookback", 0); args.setdefault("max_iters", MAXIT)
    x, y, s, iters, status, resid = eng.solve(A_bm, q_t, make_settings(args), warm=warm, P_bm=P_bm, wave=wave)
    torch.cuda.synchronize()
    assert eng.last_path == "per_instance" and eng.last_forward_kernel == ("k_fwd_wave_qp" if wave else None)
    return dict(x=x.cpu().numpy(), y=y.cpu().numpy(), s=s.cpu().numpy(), iters=iters.cpu().numpy(), status=status.cpu().numpy(), t=(x, y, s, iters, status))


def _parity(n, cones, variant, eps, lookback):
    from oracle import oracle
    tpl, A, b, c, Pm, eng, A_bm, q_t, P_bm = _case(n, cones, variant)
    assert eng.wave_qp_plan()[0] >= 0 and eng.wave_qp_plan()[1] > 0 and eng.wave_plan() == (-1, 0)
    ref = oracle.solve_batch(A, b, c, cones, P=Pm, eps=eps, max_iters=MAXIT, acceleration_lookback=lookback)
    assert (ref["status"] == 1).all() and (ref["s"][:, cones["z"]:cones["z"] + cones["l"]] < 1e-6).any()          # solved by the oracle alone, some bounds active
    what = f"n={n} {variant} eps={eps:g} aa={lookback}"
    got = _solve(eng, A_bm, q_t, P_bm, True, eps=eps, acceleration_lookback=lookback)
    _same(got, ref, eps=eps, what="wave vs oracle " + what)
    _same(got, _solve(eng, A_bm, q_t, P_bm, False, eps=eps, acceleration_lookback=lookback), eps=eps, what="wave vs ce_solve_qp " + what)


@pytest.mark.parametrize("lookback", [0, 1])
@pytest.mark.parametrize("n,cones", SHAPES, ids=[f"n{n}m{P.cone_rows(c)}" for n, c in SHAPES])
def test_every_shape_against_the_oracle_and_ce_solve_qp(n, cones, lookback):
    _parity(n, cones, "pd_upper", 1e-8, lookback)


@pytest.mark.parametrize("eps,lookback", [(1e-4, 1), (1e-8, 0)])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_p_variant_against_the_oracle_and_ce_solve_qp(variant, eps, lookback):
    _parity(*MIXED, variant, eps, lookback)


def test_warm_start_from_the_solution_takes_fewer_iterations():
    tpl, A, b, c, Pm, eng, A_bm, q_t, P_bm = _case(*MID)
    cold = _solve(eng, A_bm, q_t, P_bm, True, eps=1e-8)
    warm = _solve(eng, A_bm, q_t, P_bm, True, eps=1e-8, warm=cold["t"][:3])
    assert (warm["status"] == 1).all() and (warm["iters"] < cold["iters"]).all(), (warm["iters"], cold["iters"])
    np.testing.assert_allclose(warm["x"], cold["x"], atol=1e-6)


def _raw_solve(eng, tpl, B, A_ptr, sk, sb, q_t, P_ptr, fill=None):
    """ce_solve_qp_wave itself; fill: the value the outputs hold before the call"""
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    L, st = _lib.lib(), make_settings(dict(eps=1e-8, max_iters=MAXIT, acceleration_lookback=0))
    new = (lambda *sh, **kw: torch.empty(*sh, device="cuda", **kw)) if fill is None else (lambda *sh, **kw: torch.full(*sh, fill, device="cuda", **kw))
    x, y = new((B, tpl.n), dtype=torch.float64), new((B, tpl.m), dtype=torch.float64)
    s, it = y.clone(), new((B,), dtype=torch.int32)
    stt = it.clone()
    rc = L.ce_solve_qp_wave(eng._h, B, A_ptr, sk, sb, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), P_ptr, C.byref(st), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                            it.data_ptr(), stt.data_ptr(), None, eng._stream())
    torch.cuda.synchronize()
    return rc, (x, y, s, it, stt)


def test_batch_minor_values_give_the_same_bits():
    tpl, A, b, c, Pm, eng, A_bm, q_t, P_bm = _case(*MID)
    A_minor = A_bm.t().contiguous()          # (nnz_aug, B) contiguous: sA_k = B, sA_b = 1
    rc0, major = _raw_solve(eng, tpl, B0, A_bm.data_ptr(), 1, tpl.nnz_aug, q_t, P_bm.data_ptr())
    rc1, minor = _raw_solve(eng, tpl, B0, A_minor.data_ptr(), B0, 1, q_t, P_bm.data_ptr())
    assert rc0 == 0 == rc1, _lib.lib().ce_last_error()
    assert (major[4] == 1).all() and all(torch.equal(a_, b_) for a_, b_ in zip(major, minor))


def test_batch_edges_and_purity_under_permutation():
    """an instance's bits depend neither on its position nor on its neighbours"""
    tpl, A, b, c, Pm, eng, A_bm, q_t, P_bm = _case(*MID, B=65)
    full = _solve(eng, A_bm, q_t, P_bm, True, eps=1e-8, acceleration_lookback=1)["t"]
    assert (full[4] == 1).all()
    one = _solve(eng, A_bm[:1].contiguous(), q_t[:, :1].contiguous(), P_bm[:1].contiguous(), True, eps=1e-8, acceleration_lookback=1)["t"]
    perm = torch.from_numpy(np.random.default_rng(3).permutation(65)).cuda()
    got = _solve(eng, A_bm[perm].contiguous(), q_t[:, perm].contiguous(), P_bm[perm].contiguous(), True, eps=1e-8, acceleration_lookback=1)["t"]
    for o_, g_, f_ in zip(one, got, full):
        assert torch.equal(o_, f_[:1]) and torch.equal(g_, f_[perm])


def test_indefinite_p_fails_that_instance_alone():
    n, cones = 4, dict(z=1, l=0, q=[])
    tpl, struct = P.dense_template(n, cones), _upper_structure(n)
    eng = qp_engine(tpl, struct)
    Pm = np.stack([np.eye(n), np.diag([1.0, -1.0, 1.0, 1.0])])          # min 1/2 |x|^2, sum x = 1 beside an indefinite neighbour
    got = _solve(eng, *device_values(tpl, np.ones((2, 1, n)), np.ones((2, 1)), np.zeros((2, n)), Pm, struct), True, eps=1e-8)
    assert list(got["status"]) == [1, -4]
    assert all(np.isnan(got[k][1]).all() and np.isfinite(got[k][0]).all() for k in ("x", "y", "s"))
    np.testing.assert_allclose(got["x"][0], np.full(n, 1.0 / n), atol=1e-6)


def test_refusals_name_the_reason_and_write_nothing():
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings
    dev = torch.device("cuda", 0)
    for n, cones, with_p, word in ((4, dict(z=0, l=6, q=[]), False, "without a P structure"), (4, dict(z=0, l=3, q=[], ep=1), True, "exponential"),
                                   (33, dict(z=0, l=40, q=[]), True, "n > 32")):
        tpl = P.dense_template(n, cones)
        eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, dev, p_structure=_diag_structure(n)[:2] if with_p else None)
        assert eng.wave_qp_plan() == (-1, 0)
        A = torch.ones((3, tpl.nnz_aug), dtype=torch.float64, device="cuda"); q = torch.ones((n + 1, 3), dtype=torch.float64, device="cuda")
        Pv = torch.ones((3, n), dtype=torch.float64, device="cuda")
        rc, outs = _raw_solve(eng, tpl, 3, A.data_ptr(), 1, tpl.nnz_aug, q, Pv.data_ptr(), fill=7)
        assert rc == -2 and word in _lib.lib().ce_last_error().decode(), (rc, _lib.lib().ce_last_error())
        assert all(bool((t == 7).all()) for t in outs)
        if with_p and eng.qp_native:
            with pytest.raises(Exception, match="ce_solve_qp_wave"):
                eng.solve(A, q, make_settings({}), P_bm=Pv, wave=True)
    tpl, A, b, c, Pm, eng, A_bm, q_t, P_bm = _case(*MID)          # a served handle without P values
    rc, outs = _raw_solve(eng, tpl, B0, A_bm.data_ptr(), 1, tpl.nnz_aug, q_t, None, fill=7)
    assert rc == -1 and all(bool((t == 7).all()) for t in outs)


def test_retention_for_the_adjoint():
    """ce_vjp_qp with A_vals == NULL after the wave solve reads the rows the solve retained"""
    tpl, A, b, c, Pm, eng, A_bm, q_t, P_bm = _case(*MID)
    L = _lib.lib()
    x, y, s, _, status = _solve(eng, A_bm, q_t, P_bm, True, eps=1e-8)["t"]
    rng = np.random.default_rng(11)
    dx = torch.from_numpy(rng.standard_normal((B0, tpl.n))).cuda(); dy = torch.from_numpy(rng.standard_normal((B0, tpl.m))).cuda()
    outs = []
    for ptr in (A_bm.data_ptr(), None):
        dA = torch.empty((B0, tpl.nnz_aug), dtype=torch.float64, device="cuda"); dq = torch.empty((tpl.n + 1, B0), dtype=torch.float64, device="cuda")
        dP = torch.empty_like(P_bm); adj = torch.empty((B0,), dtype=torch.int32, device="cuda")
        rc = L.ce_vjp_qp(eng._h, B0, ptr, 1, tpl.nnz_aug, P_bm.data_ptr(), x.data_ptr(), y.data_ptr(), s.data_ptr(), dx.data_ptr(), dy.data_ptr(),
                         dA.data_ptr(), 1, tpl.nnz_aug, dq.data_ptr(), B0, 1, dP.data_ptr(), adj.data_ptr(), eng._stream())
        assert rc == 0, L.ce_last_error()
        torch.cuda.synchronize()
        outs.append((dA, dq, dP, adj))
    assert all(torch.equal(a_, b_) for a_, b_ in zip(*outs))

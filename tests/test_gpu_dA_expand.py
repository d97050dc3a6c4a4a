"""Batch-minor dA behind the search-free adjoint (csrc/ce_layout_kernels.h k_expand_dA; cone_engine.hip ce_vjp_qp): the adjoint stores only r_y per instance
(k_backward_ns's factor mode) and ONE streaming kernel expands (x, y, -dq, r_y) into the caller's (nnz_aug, B) buffer, instead of a batch-major row per instance
and a layout pass over it.  Both kernels evaluate the entry through one helper (csrc/ce_dA_entry.h), so the yardstick is exact: every case calls ConeEngine.vjp
twice on the same inputs -- batch_minor_out=True (the expansion) and batch_minor_out=False (the batch-major path, untouched) -- and the two dA must be EQUAL, bit
for bit, and dq and adj_status with them.  Shapes: the smallest at which the tiling can go wrong (a tile is 32 instances, a slab at least 256 entries)."""
import numpy as np
import pytest
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from test_gpu_parity import gpu_solve

pytestmark = pytest.mark.gpu


def _twins(eng, A_bm, x, y, s, seed, q_t, path="per_instance"):
    """the same call in both output layouts; returns the batch-minor call's (dA, dq, adj) after asserting that its twin's are the same bits"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dx = torch.randn(x.shape, dtype=torch.float64, generator=g).cuda()
    dy = torch.randn(y.shape, dtype=torch.float64, generator=g).cuda()
    dA_n, dq_n, adj_n = eng.vjp(A_bm, x, y, s, dx, dy, batch_minor_out=True, path=path, q_eval=q_t)
    dA_o, dq_o, adj_o = eng.vjp(A_bm, x, y, s, dx, dy, batch_minor_out=False, path=path, q_eval=q_t)
    torch.cuda.synchronize()
    assert dA_n.is_contiguous() and tuple(dA_n.shape) == (eng.nnz_aug, x.shape[0]) == tuple(dA_o.shape)
    assert torch.equal(adj_n, adj_o), (adj_n, adj_o)
    assert torch.equal(dq_n, dq_o)
    diff = (dA_n != dA_o)
    assert torch.equal(dA_n, dA_o), (int(diff.sum()), diff.nonzero()[:8])
    return dA_n, dq_n, adj_n


def _solved(tpl, A, b, c, eps=1e-9):
    eng, A_bm, x, y, s, iters, status, resid = gpu_solve(tpl, A, b, c, eps=eps, max_iters=200000)
    assert (status == 1).mean() > 0.9, status
    _, q_eval = tpl.values_from_dense(A, b, c)
    return eng, A_bm, x, y, s, torch.from_numpy(q_eval).cuda()


@pytest.mark.parametrize("B", [1, 33, 70])
def test_dense_metric_template_below_a_tile_one_past_it_and_across_two(B):
    cfg = P.CONFIGS["M"]
    tpl = P.dense_template(cfg["n"], cfg["cones"])
    A, b, c = P.generate(cfg["n"], cfg["cones"], B, seed=21)
    eng, A_bm, x, y, s, q_t = _solved(tpl, A, b, c)
    assert _lib.lib().ce_adjoint_ns_variant(eng._h) >= 0
    dA, dq, adj = _twins(eng, A_bm, x, y, s, 22, q_t)
    assert torch.isfinite(dA).all() and (adj == 0).float().mean() > 0.9


def test_tiny_dense_template_far_below_one_slab():
    n, cones, B = 3, {"z": 0, "l": 2, "q": [3]}, 5
    tpl = P.dense_template(n, cones)
    assert tpl.nnz_aug == 20
    A, b, c = P.generate(n, cones, B, seed=23)
    eng, A_bm, x, y, s, q_t = _solved(tpl, A, b, c)
    assert _lib.lib().ce_adjoint_ns_variant(eng._h) >= 0
    dA, _, _ = _twins(eng, A_bm, x, y, s, 24, q_t)
    assert torch.isfinite(dA).all()


def _sparse_batch(n, cones, B, seed):
    """A sparse structural pattern of A (no empty row or column) and a sparse b: rows whose b entry is structurally zero are nonnegative rows with
    a_i . x0 < 0 and s0_i = -a_i . x0, so the batch stays strictly feasible on both sides like problems.generate's.  In the template's value order (CSC of [A | b])
    neither the columns of A nor the b column are dense runs, and the position of a row's b entry is not its row index."""
    rng = np.random.default_rng(seed)
    m = P.cone_rows(cones)
    pat = rng.random((m, n)) < 0.45
    pat[np.arange(m), rng.integers(0, n, m)] = True
    pat[rng.integers(0, m, n), np.arange(n)] = True
    z, l = cones["z"], cones["l"]
    b_pat = np.ones(m, dtype=bool)
    b_pat[z + np.arange(0, l, 2)] = False
    A = (rng.standard_normal((m, n))[None] + 0.1 * rng.standard_normal((B, m, n))) / np.sqrt(n) * pat[None]
    x0 = rng.standard_normal((B, n))
    s0, y0 = P._interior_point(rng, cones, B)
    Ax = np.einsum("bij,bj->bi", A, x0)
    for r in np.nonzero(~b_pat)[0]:
        flip = Ax[:, r] > 0
        A[flip, r] *= -1.0
    Ax = np.einsum("bij,bj->bi", A, x0)
    s0[:, ~b_pat] = -Ax[:, ~b_pat]
    b = Ax + s0
    assert (b[:, ~b_pat] == 0).all() and (s0[:, ~b_pat] > 0).all()
    c = -np.einsum("bij,bi->bj", A, y0)
    return P.dense_template(n, cones, pattern=pat, b_pattern=b_pat), A, b, c


def test_sparse_template_with_a_sparse_b_column():
    n, cones, B = 12, {"z": 2, "l": 8, "q": [4, 6]}, 40
    tpl, A, b, c = _sparse_batch(n, cones, B, seed=25)
    assert tpl.m == 20 and tpl.m <= tpl.nnz_aug < (n + 1) * tpl.m * 0.7
    eng, A_bm, x, y, s, q_t = _solved(tpl, A, b, c)
    assert _lib.lib().ce_adjoint_ns_variant(eng._h) >= 0
    dA, _, _ = _twins(eng, A_bm, x, y, s, 26, q_t)
    assert torch.isfinite(dA).all()


def test_regular_and_resolved_instances_inside_one_tile():
    """nonneg-only programs (tests/test_gpu_ns_adjoint.py's LP family): the solution is a vertex, n active rows, regular.  Every third instance gets an active row
    copied over an inactive one: the vertex stays, n + 1 rows pass through it, the adjoint system is rank deficient by counting, the elimination flags it and the
    LSQR launch overwrites its whole batch-major row (status bits 4 | 8).  The expansion must copy those rows and expand their neighbours, inside the same tile of
    32.  The active-row counts are the oracle's, checked on the CPU before anything runs on the GPU; the adjoint is taken at the oracle's point, so the kernel
    counts the same rows."""
    from oracle import oracle
    n, cones, B = 8, {"z": 0, "l": 24, "q": []}, 48
    A, b, c = P.generate(n, cones, B, seed=9)
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)
    v = ref["y"] - ref["s"]
    deg = np.arange(B) % 3 == 1
    for i in np.nonzero(deg)[0]:
        ra, ri = np.argmax(v[i]), np.argmin(v[i])
        A[i, ri] = A[i, ra]; b[i, ri] = b[i, ra]
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)
    assert (ref["status"] == 1).all()
    act = ((ref["y"] - ref["s"]) > 0).sum(axis=1)
    assert (act[deg] > n).all() and (act[~deg] == n).all(), act
    assert deg[:32].any() and (~deg[:32]).any()
    tpl = P.dense_template(n, cones)
    eng, A_bm, *_ = gpu_solve(tpl, A, b, c, eps=1e-10, max_iters=200000)
    assert _lib.lib().ce_adjoint_ns_variant(eng._h) >= 0
    xr, yr, sr = (torch.from_numpy(ref[k]).cuda() for k in ("x", "y", "s"))
    _, q_eval = tpl.values_from_dense(A, b, c)
    dA, dq, adj = _twins(eng, A_bm, xr, yr, sr, 27, torch.from_numpy(q_eval).cuda())
    a = adj.cpu().numpy()
    assert ((a[deg] & 8) != 0).all() and (a[~deg] == 0).all(), a
    assert ((a[:32] & 8) != 0).any() and (a[:32] == 0).any()
    assert torch.isfinite(dA).all()


def test_without_q_eval_the_pivoting_kernel_and_the_layout_pass_still_serve_batch_minor_output():
    """q_eval=None: no re-solve is armed, k_backward_rt runs and the expansion must stay out of the way -- the batch-minor result is the layout pass's, equal to its
    batch-major twin, and right: within 1e-6 of the search-free path's on the instances neither elimination flags (tests/test_gpu_ns_adjoint.py's bound)."""
    n, cones, B = 12, {"z": 2, "l": 6, "q": [4, 5]}, 40
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=28)
    eng, A_bm, x, y, s, q_t = _solved(tpl, A, b, c)
    dA_rt, dq_rt, adj_rt = _twins(eng, A_bm, x, y, s, 29, None)
    dA_ns, dq_ns, adj_ns = _twins(eng, A_bm, x, y, s, 29, q_t)
    reg = ((adj_rt == 0) & (adj_ns == 0)).cpu().numpy()
    assert reg.mean() > 0.8
    got, want = dA_rt.cpu().numpy()[:, reg], dA_ns.cpu().numpy()[:, reg]
    assert (np.abs(got - want).max(axis=0) / (1 + np.abs(want).max(axis=0))).max() < 1e-6

"""k_bwd_wave_many (ce_vjp_many_wave, ce_vjp_many_params_wave): K cotangents of a small template, one wave per (instance, chunk of KC), at the planted points of
tests/test_gpu_bwd_wave.py (its SHAPES, case() and errors(), its bound 1e-9 = cond 3.3e3 x 2^-53 x 96 x 10: the same points, the same linear system) against the
oracle's dense elimination per cotangent.  K = 1, KC and KC + 1 of the served row: one lane, a full chunk, and a second wave with one cotangent."""
import numpy as np
import pytest
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_bwd_wave import B, BOUND, SHAPES, case, errors
from test_gpu_ns_mode_edges import _boundary

pytestmark = pytest.mark.gpu

NAMES = ["lp_vertex", "row0_full", "row1_first", "row2_full", "vertex_full", "many_small", "one_cone_full"]
CHUNK = {0: 8, 1: 16, 2: 16}          # KC of the variant list's rows
_MANY: dict = {}


def many(name, duplicate_row=False):
    """KC + 1 seeded Gaussian cotangents of a shape on the device and the oracle's dense answer to each: built once, shared, not changed"""
    key = (name, duplicate_row)
    if key not in _MANY:
        from oracle import oracle
        c = case(name, duplicate_row)
        pt, kc = c["pt"], c["eng"].bwd_wave_many_plan()[2]
        rng = np.random.default_rng(41)
        dx, dy = rng.standard_normal((kc + 1,) + pt["x"].shape), rng.standard_normal((kc + 1,) + pt["y"].shape)
        want = [oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], SHAPES[name][1], pt["x"], pt["y"], pt["s"], dx[k], dy[k], mode="dense") for k in range(kc + 1)]
        _MANY[key] = dict(kc=kc, dx=torch.from_numpy(dx).cuda(), dy=torch.from_numpy(dy).cuda(),
                          want=[dict(n=c["n"], wantA=_boundary(c["tpl"], g, c["n"]).T, wantc=g["dc"]) for g in want])
    return _MANY[key]


def run(c, dx, dy, **kw):
    A, x, y, s = c["dev"][:4]
    return c["eng"].vjp_many(A, x, y, s, dx, dy, path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"], **kw)


@pytest.mark.parametrize("which", ["one", "chunk", "chunk_plus_one"])
@pytest.mark.parametrize("name", NAMES)
def test_against_the_dense_elimination(name, which):
    c, mc = case(name), many(name)
    eng, n, kc = c["eng"], c["n"], mc["kc"]
    variant, lds, chunk = eng.bwd_wave_many_plan()
    assert variant == eng.bwd_wave_plan()[0] and chunk == CHUNK[variant] == kc and lds > eng.bwd_wave_plan()[1]
    K = {"one": 1, "chunk": kc, "chunk_plus_one": kc + 1}[which]
    dA, dq, adj = run(c, mc["dx"][:K], mc["dy"][:K], wave=True)
    assert eng.last_vjp_kernel == "ce_vjp_many_wave" and eng.last_adjoint_kernel == "k_bwd_wave_many" and dA.shape == (K, B, eng.nnz_aug)
    _, _, adj_ref = run(c, mc["dx"][:K], mc["dy"][:K])
    assert eng.last_vjp_kernel == "ce_vjp_many" and eng.last_adjoint_kernel is None
    torch.cuda.synchronize()
    assert (adj.cpu().numpy() == 0).all() and (adj_ref.cpu().numpy() == 0).all()
    for k in range(K):
        eA, ec = errors(mc["want"][k], dA[k].t(), dq[k].t())
        print(f"{name} K={K} k={k}: dA max {eA.max():.3e} dc max {ec.max():.3e} (bound {BOUND:.0e})")
        assert eA.max() < BOUND and ec.max() < BOUND, (k, eA.max(), ec.max())
    assert np.abs(dq.cpu().numpy()[:, :, n]).max() == 0


def test_without_dy():
    from oracle import oracle
    c, mc = case("row1_first"), many("row1_first")
    pt = c["pt"]
    dA, dq, adj = run(c, mc["dx"][:2], None, wave=True)
    torch.cuda.synchronize()
    assert (adj.cpu().numpy() == 0).all()
    for k in range(2):
        g = oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], SHAPES["row1_first"][1], pt["x"], pt["y"], pt["s"], mc["dx"][k].cpu().numpy(), np.zeros_like(pt["y"]), mode="dense")
        eA, ec = errors(dict(n=c["n"], wantA=_boundary(c["tpl"], g, c["n"]).T, wantc=g["dc"]), dA[k].t(), dq[k].t())
        assert eA.max() < BOUND and ec.max() < BOUND, (k, eA.max(), ec.max())


def test_a_cotangent_depends_on_neither_its_lane_nor_its_chunk_nor_the_instances_position():
    c, mc = case("row1_full"), many("row1_full")
    kc = mc["kc"]
    dx, dy = (torch.cat([t[:kc], t[:1]]).contiguous() for t in (mc["dx"], mc["dy"]))          # cotangent 0 again, alone in the second chunk
    base = run(c, dx, dy, wave=True)
    assert all(torch.equal(o[0], o[kc]) for o in base)
    shifted = run(c, dx[1:].contiguous(), dy[1:].contiguous(), wave=True)          # every cotangent one lane lower
    assert all(torch.equal(o, b[1:]) for o, b in zip(shifted, base))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(B)).cuda()
    inv = torch.argsort(perm)
    cp = dict(c, dev=[t[perm].contiguous() for t in c["dev"]], q=c["q"][:, perm].contiguous())
    got = run(cp, dx[:, perm].contiguous(), dy[:, perm].contiguous(), wave=True)
    assert all(torch.equal(o[:, inv], b) for o, b in zip(got, base))


def test_a_redundant_equality_row_is_flagged_once_and_resolved_for_every_cotangent():
    from oracle import oracle
    c, mc = case("row1_full", duplicate_row=True), many("row1_full", duplicate_row=True)
    pt, n, kc = c["pt"], c["n"], mc["kc"]
    dA, dq, adj = run(c, mc["dx"], mc["dy"], wave=True)          # KC + 1 cotangents: two waves flag each odd instance
    torch.cuda.synchronize()
    odd = np.arange(B) % 2 == 1
    assert (adj.cpu().numpy() == np.where(odd, 12, 0)[None, :]).all(), adj
    for k in (0, kc):          # one cotangent of each chunk against the oracle's LSQR (test_gpu_bwd_wave.py's tolerance), the even instances against its dense answer
        eA, ec = errors(mc["want"][k], dA[k].t(), dq[k].t())
        assert eA[~odd].max() < BOUND and ec[~odd].max() < BOUND
        g = oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], pt["cones"], pt["x"], pt["y"], pt["s"], mc["dx"][k].cpu().numpy(), mc["dy"][k].cpu().numpy(), mode="lsqr",
                                 lsqr_atol=TIGHT_LSQR[0], lsqr_btol=TIGHT_LSQR[1], lsqr_iter_lim=TIGHT_LSQR[2])
        want, got = _boundary(c["tpl"], g, n)[:, odd], dA[k].t().cpu().numpy()[:, odd]
        print(f"k={k} odd instances against the oracle's LSQR: dA {np.abs(got - want).max() / (1 + np.abs(want).max()):.3e} (bound 1e-6)")
        assert np.abs(got - want).max() < 1e-6 * (1 + np.abs(want).max())
        assert np.abs(dq[k].t().cpu().numpy()[:n, odd] - g["dc"].T[:, odd]).max() < 1e-6 * (1 + np.abs(g["dc"]).max())


def test_record_mode_against_the_maps_applied_to_the_dA_route():
    from cvxpylayers_amd.interfaces.param_grad import ComposedMaps
    from cvxpylayers_amd.torch.cvxpylayer import _DeviceCSR, _spmm_bm
    from test_gpu_param_grad import synthetic_maps
    c, mc = case("lp_vertex"), many("lp_vertex")          # (n = 2: the smallest shape; the "own" maps end in a constant row with five entries)
    eng, tpl, K = c["eng"], c["tpl"], mc["kc"] + 1
    Am, qm = synthetic_maps(tpl, seed=3)["own"]
    dA, dq, adj = run(c, mc["dx"], mc["dy"], wave=True)
    g_ref = torch.zeros((K * B, Am.shape[0]), dtype=torch.float64, device="cuda")
    _spmm_bm(_DeviceCSR(Am).on(dA.device)[0], dA.view(K * B, -1), out=g_ref)
    _spmm_bm(_DeviceCSR(qm).on(dA.device)[0], dq.view(K * B, -1), out=g_ref)
    A, x, y, s = c["dev"][:4]
    g, dq_p, adj_p = eng.vjp_many_params(A, x, y, s, mc["dx"], mc["dy"], ComposedMaps(Am, qm, tpl.indices, tpl.indptr, tpl.n, tpl.m), lsqr=TIGHT_LSQR, q_eval=c["q"], wave=True)
    assert eng.last_vjp_kernel == "ce_vjp_many_params_wave" and eng.last_adjoint_kernel == "k_bwd_wave_many"
    torch.cuda.synchronize()
    assert torch.equal(dq_p, dq) and torch.equal(adj_p, adj)
    single = (np.diff(Am.indptr) + np.diff(qm.indptr)) == 1
    gn, grn = g.cpu().numpy().reshape(K * B, -1), g_ref.cpu().numpy()
    assert single.any() and not single.all() and np.array_equal(gn[:, single], grn[:, single])
    assert np.abs(gn - grn).max() < BOUND * (1 + np.abs(grn).max())


@pytest.mark.parametrize("entry", ["ce_vjp_many_wave", "ce_vjp_many_params_wave"])
def test_refusals_leave_the_outputs_untouched(entry):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    c, L = case("row1_full"), _lib.lib()
    tpl = P.dense_template(4, dict(z=0, l=3, q=[], ep=1, p=[]))
    exp_eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))
    assert exp_eng.bwd_wave_many_plan() == (-1, 0, 0)
    for eng, q, why in ((exp_eng, c["q"], "exponential"), (c["eng"], None, "q_vals == NULL")):
        f64 = dict(dtype=torch.float64, device="cuda")
        K = 3
        A, x, y, s = (torch.zeros((2, k), **f64) for k in (eng.nnz_aug, eng.n, eng.m, eng.m))
        dx, dy = torch.zeros((K, 2, eng.n), **f64), torch.zeros((K, 2, eng.m), **f64)
        out, dq, adj = torch.full((K, 2, eng.nnz_aug), 7.0, **f64), torch.full((K, 2, eng.n + 1), 7.0, **f64), torch.full((K, 2), 7, dtype=torch.int32, device="cuda")
        maps = [torch.zeros(2, dtype=torch.int32, device="cuda") for _ in range(3)] + [torch.zeros(2, **f64)]
        head = (eng._h, 2, K, A.data_ptr(), eng.nnz_aug, q.data_ptr() if q is not None else None, 2 if q is not None else 0, 1 if q is not None else 0,
                x.data_ptr(), y.data_ptr(), s.data_ptr(), dx.data_ptr(), dy.data_ptr())
        tail = (out.data_ptr(), dq.data_ptr(), adj.data_ptr(), None)
        rc = getattr(L, entry)(*head, *((1, *(t.data_ptr() for t in maps)) if "params" in entry else ()), *tail)
        torch.cuda.synchronize()
        msg = L.ce_last_error().decode()
        assert rc == -2 and entry + ":" in msg and why in msg, (rc, msg)
        assert (out == 7).all() and (dq == 7).all() and (adj == 7).all()
    with pytest.raises(Exception, match="ce_vjp_many_wave"):
        exp_eng.vjp_many(A, x, y, s, dx, dy, path="per_instance", q_eval=c["q"][:, :2].contiguous(), wave=True)

"""k_bwd_wave (ce_vjp_wave): the adjoint of a small template, one instance per wave, at planted KKT points (tests/ns_edge_kit.plant, kind "plain", B = 24, seed 3)
against the oracle's dense elimination, compared as tests/test_gpu_ns_mode_edges.py compares: entries through the template's pattern, per instance
max |got - want| / (1 + max |want|).  Every planted instance is regular (cond(J) <= 3.3e3, KKT residual <= 1e-15), so every status is 0 -- ce_vjp's too -- and the bound
is 1e-9 = cond 3.3e3 x 2^-53 x (n + m = 96) x 10.  The shapes sit on both sides of every row of the variant list and at the ends of every loop of the kernel:
nf = 0 (no Hessian), neq = 1 (the largest sweep), neq = n (the largest row elimination), cones of dimension 1 and 2, twenty boundary cones in one wave."""
import numpy as np
import pytest
import torch

import ns_edge_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_ns_mode_edges import _boundary, _rel

pytestmark = pytest.mark.gpu

BOUND, B = 1e-9, 24
SHAPES = {          # name: (n, cones, states)
    "lp_vertex": (2, dict(z=1, l=2, q=[]), ()),
    "tiny_soc": (2, dict(z=0, l=1, q=[2]), ("bd",)),
    "row0_full": (8, dict(z=2, l=6, q=[8]), ("bd",)),
    "row1_first": (9, dict(z=2, l=7, q=[8]), ("bd",)),
    "row1_full": (16, dict(z=2, l=10, q=[4, 16]), ("in", "bd")),
    "row2_first": (17, dict(z=2, l=11, q=[4, 16]), ("in", "bd")),
    "row2_full": (32, dict(z=4, l=20, q=[1, 2, 5, 32]), ("in", "bd", "out", "bd")),
    "one_cone": (12, dict(z=0, l=0, q=[24]), ("bd",)),
    "one_cone_full": (32, dict(z=0, l=0, q=[64]), ("bd",)),
    "vertex_full": (32, dict(z=8, l=56, q=[]), ()),
    "many_small": (32, dict(z=1, l=3, q=[3] * 20), ("bd",) * 20),
    "wide": (32, dict(z=8, l=24, q=[16, 16]), ("bd", "out")),
}
_CASES: dict = {}


def case(name, duplicate_row=False):
    """the planted batch of a shape on the device, Gaussian cotangents and the oracle's dense reference: built once per name, shared, not changed"""
    key = (name, duplicate_row)
    if key not in _CASES:
        from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
        from oracle import oracle
        n, cones, states = SHAPES[name]
        pt = dict(K.plant(("plain", n, cones, states), B=B, seed=3))
        if duplicate_row:          # the first zero row again in the second on the odd instances (b likewise: s = 0 there), c = -A^T y with it
            A, b = pt["A"].copy(), pt["b"].copy()
            A[1::2, 1] = A[1::2, 0]; b[1::2, 1] = b[1::2, 0]
            pt.update(A=A, b=b, c=-np.einsum("bij,bi->bj", A, pt["y"]))
        tpl = P.dense_template(n, cones)
        eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))
        A_eval, q_eval = tpl.values_from_dense(pt["A"], pt["b"], pt["c"])
        rng = np.random.default_rng(31)
        cot = rng.standard_normal(pt["x"].shape), rng.standard_normal(pt["y"].shape)
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (A_eval.T, pt["x"], pt["y"], pt["s"], *cot)]
        g = oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], cones, pt["x"], pt["y"], pt["s"], *cot, mode="dense")
        _CASES[key] = dict(pt=pt, tpl=tpl, eng=eng, n=n, dev=dev, q=torch.from_numpy(q_eval).cuda(), cot=cot, wantA=_boundary(tpl, g, n).T, wantc=g["dc"])
    return _CASES[key]


def errors(c, dA, dq):
    return _rel(dA.cpu().numpy().T, c["wantA"]), _rel(dq.cpu().numpy()[:c["n"]].T, c["wantc"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_dense_elimination(name):
    c = case(name)
    eng, n = c["eng"], c["n"]
    assert eng.bwd_wave_plan()[0] == next(v for v, (nx, my) in enumerate([(8, 16), (16, 32), (32, 64)]) if n <= nx and eng.m <= my)
    dA, dq, adj = eng.vjp(*c["dev"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"], wave=True)
    assert eng.last_adjoint_kernel == "k_bwd_wave"
    _, _, adj_ref = eng.vjp(*c["dev"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"])
    assert eng.last_adjoint_kernel is None
    torch.cuda.synchronize()
    eA, ec = errors(c, dA, dq)
    print(f"{name}: dA max {eA.max():.3e} dc max {ec.max():.3e} (bound {BOUND:.0e}) status {np.bincount(adj.cpu().numpy()).tolist()}")
    assert (adj_ref.cpu().numpy() == 0).all() and (adj.cpu().numpy() == 0).all()
    assert eA.max() < BOUND and ec.max() < BOUND, (eA.max(), ec.max())
    assert np.abs(dq.cpu().numpy()[n]).max() == 0
    dA_t, dq_t, adj_t = eng.vjp(*c["dev"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"], wave=True, batch_minor_out=True)          # the factor mode + k_expand_dA
    assert dA_t.is_contiguous() and torch.equal(dA_t, dA.contiguous()) and torch.equal(dq_t, dq) and torch.equal(adj_t, adj)


def test_an_instance_does_not_depend_on_its_position():
    c = case("row1_full")
    eng = c["eng"]
    base = eng.vjp(*c["dev"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"], wave=True)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(B)).cuda()
    inv = torch.argsort(perm)
    got = eng.vjp(*(t[perm].contiguous() for t in c["dev"]), path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"][:, perm].contiguous(), wave=True)
    one = eng.vjp(*(t[5:6].contiguous() for t in c["dev"]), path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"][:, 5:6].contiguous(), wave=True)
    assert torch.equal(got[0][:, inv], base[0]) and torch.equal(got[1][:, inv], base[1]) and torch.equal(got[2][inv], base[2])
    assert torch.equal(one[0][:, 0], base[0][:, 5]) and torch.equal(one[1][:, 0], base[1][:, 5]) and int(one[2][0]) == int(base[2][5])


def test_a_redundant_equality_row_is_flagged_and_resolved():
    from oracle import oracle
    c = case("row1_full", duplicate_row=True)
    pt, eng, n = c["pt"], c["eng"], c["n"]
    dA, dq, adj = eng.vjp(*c["dev"], path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"], wave=True)
    torch.cuda.synchronize()
    odd = np.arange(B) % 2 == 1
    assert (adj.cpu().numpy() == np.where(odd, 12, 0)).all(), adj
    eA, ec = errors(c, dA, dq)
    print(f"even instances: dA max {eA[~odd].max():.3e} dc max {ec[~odd].max():.3e} (bound {BOUND:.0e})")
    assert eA[~odd].max() < BOUND and ec[~odd].max() < BOUND
    g = oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], pt["cones"], pt["x"], pt["y"], pt["s"], *c["cot"], mode="lsqr",
                             lsqr_atol=TIGHT_LSQR[0], lsqr_btol=TIGHT_LSQR[1], lsqr_iter_lim=TIGHT_LSQR[2])
    want = _boundary(c["tpl"], g, n)[:, odd]
    got = dA.cpu().numpy()[:, odd]
    print(f"odd instances against the oracle's LSQR: dA {np.abs(got - want).max() / (1 + np.abs(want).max()):.3e} (bound 1e-6)")
    assert np.abs(got - want).max() < 1e-6 * (1 + np.abs(want).max())
    assert np.abs(dq.cpu().numpy()[:n, odd] - g["dc"].T[:, odd]).max() < 1e-6 * (1 + np.abs(g["dc"]).max())


def test_refusals_leave_the_outputs_untouched():
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    c, L = case("row1_full"), _lib.lib()
    tpl = P.dense_template(4, dict(z=0, l=3, q=[], ep=1, p=[]))
    exp_eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))
    assert exp_eng.bwd_wave_plan() == (-1, 0)
    for eng, q, why in ((exp_eng, c["q"], "exponential"), (c["eng"], None, "q_vals == NULL")):
        f64 = dict(dtype=torch.float64, device="cuda")
        ins = [torch.zeros((2, k), **f64) for k in (eng.nnz_aug, eng.n, eng.m, eng.m, eng.n, eng.m)]
        dA, dq, adj = torch.full((2, eng.nnz_aug), 7.0, **f64), torch.full((eng.n + 1, 2), 7.0, **f64), torch.full((2,), 7, dtype=torch.int32, device="cuda")
        rc = L.ce_vjp_wave(eng._h, 2, ins[0].data_ptr(), 1, eng.nnz_aug, q.data_ptr() if q is not None else None, 2 if q is not None else 0, 1 if q is not None else 0,
                           *(t.data_ptr() for t in ins[1:]), dA.data_ptr(), 1, eng.nnz_aug, dq.data_ptr(), 2, 1, adj.data_ptr(), None)
        torch.cuda.synchronize()
        msg = L.ce_last_error().decode()
        assert rc != 0 and "ce_vjp_wave" in msg and why in msg, (rc, msg)
        assert (dA == 7).all() and (dq == 7).all() and (adj == 7).all()
        with pytest.raises(Exception, match="ce_vjp_wave|wave"):
            eng.vjp(*ins, path="per_instance", q_eval=None if q is None else q[:, :2].contiguous(), wave=True)

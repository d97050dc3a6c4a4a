"""k_bwd_wave_qp (ce_vjp_qp_wave): the adjoint of a small template with a quadratic objective inside the kernels, one instance per wave, at planted KKT points
(tests/ns_edge_kit.plant, kind "qp", B = 24, seed 3) against the oracle's dense elimination with P, compared as tests/test_gpu_bwd_wave.py compares: dA through the
template's pattern, dc as is, dP through the P structure, per instance max |got - want| / (1 + max |want|).  Every planted instance is regular, so every status is 0
-- ce_vjp_qp's too -- and the bound is derived per case from ns_edge_kit.regularity: max(1e-9, 10 (n + m) 2^-53 max cond(J)), test_gpu_bwd_wave.py's formula (1e-9 on
every shape but row0_nf0, whose square random B has cond(J) 6.0e5: about 1.6e-8).  The shapes sit on both sides of every row of the variant list and at the ends of
every loop: neq = 0 with no weighted row (the reduced Hessian is P alone), neq = n (nothing to sweep), cones of dimension 1 and 2, twenty boundary cones in a wave."""
import numpy as np
import pytest
import torch

import ns_edge_kit as K
import qp_ns_kit as Q
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from test_gpu_ns_mode_edges import _boundary, _rel
from test_gpu_vjp_qp_many import _dp_values
from test_quad_objective import _upper_structure

pytestmark = pytest.mark.gpu

B = 24
_ROW0 = (8, dict(z=2, l=6, q=[8]), ("bd",))
SHAPES = {          # name: ((n, cones, states), plant keywords)
    "lp_vertex": ((2, dict(z=1, l=2, q=[]), ()), {}),
    "tiny_soc": ((2, dict(z=0, l=1, q=[2]), ("bd",)), {}),
    "no_active_row": ((4, dict(z=0, l=8, q=[]), ()), dict(active=0)),
    "row0_full": (_ROW0, {}),
    "row0_nf0": (_ROW0, dict(active=5)),
    "row1_first": ((9, dict(z=2, l=7, q=[8]), ("bd",)), {}),
    "row1_full": ((16, dict(z=2, l=10, q=[4, 16]), ("in", "bd")), {}),
    "row2_first": ((17, dict(z=2, l=11, q=[4, 16]), ("in", "bd")), {}),
    "row2_full": ((32, dict(z=4, l=20, q=[1, 2, 5, 32]), ("in", "bd", "out", "bd")), {}),
    "one_cone_full": ((32, dict(z=0, l=0, q=[64]), ("bd",)), {}),
    "vertex_full": ((32, dict(z=8, l=56, q=[]), ()), {}),
    "many_small": ((32, dict(z=1, l=3, q=[3] * 20), ("bd",) * 20), {}),
}
_CASES: dict = {}


def case(name, triangle=False, duplicate_row=False):
    """the planted batch of a shape on the device, Gaussian cotangents, the oracle's dense reference and the bound: built once per key, shared, not changed"""
    key = (name, triangle, duplicate_row)
    if key not in _CASES:
        from oracle import oracle
        (n, cones, states), kw = SHAPES[name]
        pt = dict(K.plant(("qp", n, cones, states), B=B, seed=3, **kw))
        cond, resid = K.regularity(pt)          # (of the point as planted: the duplicated row below is singular on purpose)
        assert resid.max() <= 1e-14
        if duplicate_row:          # the first zero row again in the second on the odd instances (b likewise: s = 0 there), c = -P x - A^T y with it
            A, b = pt["A"].copy(), pt["b"].copy()
            A[1::2, 1] = A[1::2, 0]; b[1::2, 1] = b[1::2, 0]
            pt.update(A=A, b=b, c=-np.einsum("bij,bj->bi", pt["Pm"], pt["x"]) - np.einsum("bij,bi->bj", A, pt["y"]))
        tpl = P.dense_template(n, cones)
        struct = _upper_structure(n) if triangle else Q.full_structure(n)
        eng = Q.qp_engine(tpl, struct)
        A_bm, _q, P_bm = Q.device_values(tpl, pt["A"], pt["b"], pt["c"], pt["Pm"], struct)
        rng = np.random.default_rng(31)
        cot = rng.standard_normal(pt["x"].shape), rng.standard_normal(pt["y"].shape)
        dev = [A_bm] + [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pt["x"], pt["y"], pt["s"], *cot)]
        g = oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], cones, pt["x"], pt["y"], pt["s"], *cot, P=pt["Pm"], mode="dense")
        _CASES[key] = dict(eng=eng, n=n, dev=dev, P_bm=P_bm, wantA=_boundary(tpl, g, n).T, wantc=g["dc"], wantP=_dp_values(g["dP"], struct),
                           bound=max(1e-9, 10 * (n + tpl.m) * 2.0 ** -53 * cond.max()))
    return _CASES[key]


def run(c, wave=True, sel=None, **kw):
    dev, P_bm = (c["dev"], c["P_bm"]) if sel is None else ([t[sel].contiguous() for t in c["dev"]], c["P_bm"][sel].contiguous())
    return c["eng"].vjp(*dev, path="per_instance", P_bm=P_bm, wave=wave, **kw)


def errors(c, dA, dq, dP):
    return _rel(dA.cpu().numpy().T, c["wantA"]), _rel(dq.cpu().numpy()[:c["n"]].T, c["wantc"]), _rel(dP.cpu().numpy(), c["wantP"])


@pytest.mark.parametrize("name,triangle", [(name, False) for name in SHAPES] + [("row1_full", True)])
def test_against_the_dense_elimination(name, triangle):
    c = case(name, triangle)
    eng, n = c["eng"], c["n"]
    assert eng.qp_native and eng.bwd_wave_qp_plan()[0] == next(v for v, (nx, my) in enumerate([(8, 16), (16, 32), (32, 64)]) if n <= nx and eng.m <= my)
    dA, dq, adj, dP = run(c)
    assert eng.last_adjoint_kernel == "k_bwd_wave_qp"
    ref = run(c, wave=False)
    assert eng.last_adjoint_kernel is None
    torch.cuda.synchronize()
    e, e_ref = np.stack(errors(c, dA, dq, dP)), np.stack(errors(c, *ref[:2], ref[3]))
    print(f"{name}{' (one triangle)' if triangle else ''}: dA, dc, dP max {e.max(axis=1)} against ce_vjp_qp's {e_ref.max(axis=1)} (bound {c['bound']:.1e}) "
          f"status {np.bincount(adj.cpu().numpy()).tolist()}")
    assert (ref[2].cpu().numpy() == 0).all() and (adj.cpu().numpy() == 0).all()
    assert e.max() < c["bound"], e.max(axis=1)
    assert np.abs(dq.cpu().numpy()[n]).max() == 0
    dA_t, dq_t, adj_t, dP_t = run(c, batch_minor_out=True)
    assert dA_t.is_contiguous() and torch.equal(dA_t, dA.contiguous()) and torch.equal(dq_t, dq) and torch.equal(adj_t, adj) and torch.equal(dP_t, dP)


def test_an_instance_does_not_depend_on_its_position():
    c = case("row1_full")
    base = run(c)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(B)).cuda()
    inv = torch.argsort(perm)
    got, one = run(c, sel=perm), run(c, sel=slice(5, 6))
    assert torch.equal(got[0][:, inv], base[0]) and torch.equal(got[1][:, inv], base[1]) and torch.equal(got[2][inv], base[2]) and torch.equal(got[3][inv], base[3])
    assert torch.equal(one[0][:, 0], base[0][:, 5]) and torch.equal(one[1][:, 0], base[1][:, 5]) and int(one[2][0]) == int(base[2][5]) and torch.equal(one[3][0], base[3][5])


def test_a_redundant_equality_row_is_flagged():
    """no reference for the odd instances: the two right-hand sides of the duplicated row differ, the system is inconsistent -- the flag and finiteness alone"""
    c = case("row1_full", duplicate_row=True)
    dA, dq, adj, dP = run(c)
    torch.cuda.synchronize()
    odd = np.arange(B) % 2 == 1
    assert (adj.cpu().numpy() == np.where(odd, 4, 0)).all(), adj
    assert all(bool(torch.isfinite(t).all()) for t in (dA, dq, dP))
    e = np.stack(errors(c, dA, dq, dP))[:, ~odd]
    print(f"even instances: dA, dc, dP max {e.max(axis=1)} (bound {c['bound']:.1e})")
    assert e.max() < c["bound"]


def test_refusals_leave_the_outputs_untouched():
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    L = _lib.lib()
    tpl = P.dense_template(16, dict(z=2, l=10, q=[4, 16]))
    lin = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))
    big = Q.qp_engine(P.dense_template(33, dict(z=1, l=4, q=[])), Q.full_structure(33))
    for eng, why in ((lin, "without a P structure"), (big, "n > 32")):
        assert eng.bwd_wave_qp_plan() == (-1, 0)
        f64 = dict(dtype=torch.float64, device="cuda")
        nnz_p = max(eng.nnz_p, 1)
        ins = [torch.zeros((2, k), **f64) for k in (eng.nnz_aug, nnz_p, eng.n, eng.m, eng.m, eng.n, eng.m)]
        dA, dq, dP = torch.full((2, eng.nnz_aug), 7.0, **f64), torch.full((eng.n + 1, 2), 7.0, **f64), torch.full((2, nnz_p), 7.0, **f64)
        adj = torch.full((2,), 7, dtype=torch.int32, device="cuda")
        rc = L.ce_vjp_qp_wave(eng._h, 2, ins[0].data_ptr(), 1, eng.nnz_aug, ins[1].data_ptr(), *(t.data_ptr() for t in ins[2:]), dA.data_ptr(), 1, eng.nnz_aug,
                              dq.data_ptr(), 2, 1, dP.data_ptr(), adj.data_ptr(), None)
        torch.cuda.synchronize()
        msg = L.ce_last_error().decode()
        assert rc != 0 and "ce_vjp_qp_wave" in msg and why in msg, (rc, msg)
        assert (dA == 7).all() and (dq == 7).all() and (dP == 7).all() and (adj == 7).all()

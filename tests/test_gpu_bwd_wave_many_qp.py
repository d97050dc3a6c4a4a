"""k_bwd_wave_many_qp (ce_vjp_qp_many_wave, ce_vjp_qp_many_params_wave): K cotangents through the adjoint of a small template with a quadratic objective inside the
kernels, one wave per (instance, chunk of KC cotangents), at the planted KKT points of tests/test_gpu_bwd_wave_qp.py (its SHAPES; ns_edge_kit.plant, kind "qp", B = 24,
seed 3) with KC + 1 seeded Gaussian cotangents against the oracle's dense elimination with P per cotangent.  Compared as that file compares -- dA through the
template's pattern, dc as is, dP through the structure, per instance max |got - want| / (1 + max |want|) -- under its derived bound
max(1e-9, 10 (n + m) 2^-53 max cond(J)).  K = 1 is one right-hand-side lane, K = KC a full chunk, K = KC + 1 a second wave with one cotangent."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ns_edge_kit as K
import qp_ns_kit as Q
import test_gpu_bwd_wave_qp as W
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from test_gpu_ns_mode_edges import _boundary, _rel
from test_gpu_param_grad import compare
from test_gpu_param_grad_kinds import _maps_of
from test_gpu_vjp_qp_many import _dp_values
from test_quad_objective import _upper_structure

pytestmark = pytest.mark.gpu

B = W.B
NAMES = ["lp_vertex", "no_active_row", "row0_nf0", "row1_first", "row2_full", "one_cone_full", "many_small"]
_CASES: dict = {}


def case(name, triangle=False, duplicate_row=False):
    """W.case's engine, device point and bound, KC + 1 Gaussian cotangents on the device and the oracle's answer to each: built once per key, shared, not changed"""
    key = (name, triangle, duplicate_row)
    if key not in _CASES:
        from oracle import oracle
        c = W.case(name, triangle, duplicate_row)
        (n, cones, states), kw = W.SHAPES[name]
        pt = dict(K.plant(("qp", n, cones, states), B=B, seed=3, **kw))
        if duplicate_row:          # (W.case's statement of the duplicated row)
            A, b = pt["A"].copy(), pt["b"].copy()
            A[1::2, 1] = A[1::2, 0]; b[1::2, 1] = b[1::2, 0]
            pt.update(A=A, b=b, c=-np.einsum("bij,bj->bi", pt["Pm"], pt["x"]) - np.einsum("bij,bi->bj", A, pt["y"]))
        tpl = P.dense_template(n, cones)
        struct = _upper_structure(n) if triangle else Q.full_structure(n)
        kc = c["eng"].bwd_wave_many_qp_plan()[2]
        rng = np.random.default_rng(41)
        dx, dy = rng.standard_normal((kc + 1,) + pt["x"].shape), rng.standard_normal((kc + 1,) + pt["y"].shape)
        gs = [oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], cones, pt["x"], pt["y"], pt["s"], dx[k], dy[k], P=pt["Pm"], mode="dense") for k in range(kc + 1)]
        _CASES[key] = dict(eng=c["eng"], n=n, tpl=tpl, struct=struct, kc=kc, dev=c["dev"][:4], P_bm=c["P_bm"], bound=c["bound"],
                           dx=torch.from_numpy(dx).cuda(), dy=torch.from_numpy(dy).cuda(), wantA=np.stack([_boundary(tpl, g, n).T for g in gs]),
                           wantc=np.stack([g["dc"] for g in gs]), wantP=np.stack([_dp_values(g["dP"], struct) for g in gs]))
    return _CASES[key]


def run(c, ks, wave=True, sel=slice(None)):
    A_bm, x, y, s = (t[sel].contiguous() for t in c["dev"])
    return c["eng"].vjp_many(A_bm, x, y, s, c["dx"][ks][:, sel].contiguous(), c["dy"][ks][:, sel].contiguous(), path="per_instance",
                             P_bm=c["P_bm"][sel].contiguous(), qp_many=True, wave=wave)


def errors(c, ks, dA, dq, dP):
    """(3, K, B): per cotangent and instance, dA, dc, dP"""
    dA, dq, dP = (t.cpu().numpy() for t in (dA, dq, dP))
    return np.stack([[_rel(dA[i], c["wantA"][k]), _rel(dq[i][:, :c["n"]], c["wantc"][k]), _rel(dP[i], c["wantP"][k])] for i, k in enumerate(ks)]).transpose(1, 0, 2)


@pytest.mark.parametrize("kcount", ["one", "chunk", "chunk_and_one"])
@pytest.mark.parametrize("name,triangle", [(name, False) for name in NAMES] + [("row1_full", True)])
def test_against_the_dense_elimination(name, triangle, kcount):
    c = case(name, triangle)
    eng, n, kc = c["eng"], c["n"], c["kc"]
    v = next(v for v, (nx, my) in enumerate([(8, 16), (16, 32), (32, 64)]) if n <= nx and eng.m <= my)
    assert eng.bwd_wave_many_qp_plan()[0] == v == eng.bwd_wave_qp_plan()[0] and kc == (8, 16, 8)[v]
    ks = list(range({"one": 1, "chunk": kc, "chunk_and_one": kc + 1}[kcount]))
    dA, dq, adj, dP = run(c, ks)
    assert eng.last_vjp_kernel == "ce_vjp_qp_many_wave" and eng.last_adjoint_kernel == "k_bwd_wave_many_qp" and eng.last_vjp_many_path == "many"
    ref = run(c, ks, wave=False)
    assert eng.last_vjp_kernel == "ce_vjp_qp_many" and eng.last_adjoint_kernel is None
    torch.cuda.synchronize()
    e, e_ref = errors(c, ks, dA, dq, dP), errors(c, ks, ref[0], ref[1], ref[3])
    print(f"{name}{' (one triangle)' if triangle else ''} K = {len(ks)}: dA, dc, dP max {e.max(axis=(1, 2))} against ce_vjp_qp_many's {e_ref.max(axis=(1, 2))} "
          f"(bound {c['bound']:.1e}) status {np.bincount(adj.cpu().numpy().ravel()).tolist()}")
    assert adj.shape == (len(ks), B) and (adj.cpu().numpy() == 0).all() and (ref[2].cpu().numpy() == 0).all()
    assert e.max() < c["bound"], e.max(axis=(1, 2))
    assert np.abs(dq.cpu().numpy()[..., n]).max() == 0


def test_a_cotangent_does_not_depend_on_its_lane_chunk_or_batch_position():
    c = case("row1_full")
    kc = c["kc"]
    ks = list(range(kc))
    base = run(c, ks)
    again = run(c, ks + [0])          # cotangent 0 once more, alone in the second chunk
    assert all(torch.equal(a[kc], b[0]) and torch.equal(a[:kc], b) for a, b in zip(again, base))
    rolled = run(c, ks[-1:] + ks[:-1])          # every cotangent one lane further
    assert all(torch.equal(a[1:], b[:-1]) and torch.equal(a[0], b[-1]) for a, b in zip(rolled, base))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(B)).cuda()
    got = run(c, ks, sel=perm)
    assert all(torch.equal(a[:, torch.argsort(perm)], b) for a, b in zip(got, base))


def test_a_redundant_equality_row_is_flagged_for_every_cotangent():
    """no reference for the odd instances: the two right-hand sides of the duplicated row differ, the system is inconsistent -- the flag and finiteness alone"""
    c = case("row1_full", duplicate_row=True)
    ks = list(range(c["kc"] + 1))
    dA, dq, adj, dP = run(c, ks)
    torch.cuda.synchronize()
    odd = np.arange(B) % 2 == 1
    assert (adj.cpu().numpy() == np.where(odd, 4, 0)[None]).all(), adj
    assert all(bool(torch.isfinite(t).all()) for t in (dA, dq, dP))
    e = errors(c, ks, dA, dq, dP)[:, :, ~odd]
    print(f"even instances: dA, dc, dP max {e.max(axis=(1, 2))} (bound {c['bound']:.1e})")
    assert e.max() < c["bound"]


def test_record_mode_against_this_routes_dA_dq_dP():
    from cvxpylayers_amd.torch.cvxpylayer import _spmm_bm
    c = case("lp_vertex")
    eng, ks = c["eng"], list(range(c["kc"] + 1))
    dA, dq_ref, adj_ref, dP = run(c, ks)
    for mname, mp in _maps_of(c["tpl"], c["struct"]).items():
        if "P" not in mp:
            continue
        g, dq, adj = eng.vjp_many_params(*c["dev"], c["dx"], c["dy"], mp["cm"], P_bm=c["P_bm"], qp_many=True, wave=True)
        assert eng.last_vjp_kernel == "ce_vjp_qp_many_params_wave" and eng.last_adjoint_kernel == "k_bwd_wave_many_qp"
        assert torch.equal(dq, dq_ref) and torch.equal(adj, adj_ref)
        g_ref = torch.zeros((len(ks) * B, mp["cm"].rows), dtype=torch.float64, device="cuda")
        for m_, t in ((mp["dA"], dA), (mp["dq"], dq_ref), (mp["dP"], dP)):
            _spmm_bm(m_.on(g_ref.device)[0], t.reshape(len(ks) * B, -1), out=g_ref)
        ext = dict(A=mp["A"], q=sp.csr_array(sp.hstack([mp["q"], mp["P"]])))          # (a P entry counts as a term like every other)
        compare(f"lp_vertex {mname}", g.cpu().numpy(), g_ref.view(len(ks), B, -1).cpu().numpy(), dA.cpu().numpy(), torch.cat([dq_ref, dP], dim=2).cpu().numpy(), ext)


def test_refusals_leave_the_outputs_untouched():
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    L = _lib.lib()
    tpl = P.dense_template(16, dict(z=2, l=10, q=[4, 16]))
    lin = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))
    big = Q.qp_engine(P.dense_template(33, dict(z=1, l=4, q=[])), Q.full_structure(33))
    for eng, why in ((lin, "without a P structure"), (big, "n > 32")):
        assert eng.bwd_wave_many_qp_plan() == (-1, 0, 0)
        f64 = dict(dtype=torch.float64, device="cuda")
        nnz_p = max(eng.nnz_p, 1)
        ins = [torch.zeros(sh, **f64) for sh in ((2, eng.nnz_aug), (2, nnz_p), (2, eng.n), (2, eng.m), (2, eng.m), (3, 2, eng.n), (3, 2, eng.m))]
        dA, dq, dP, g = (torch.full((3, 2, k), 7.0, **f64) for k in (eng.nnz_aug, eng.n + 1, nnz_p, 2))
        adj = torch.full((3, 2), 7, dtype=torch.int32, device="cuda")
        imap, vmap = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, **f64)
        head = (eng._h, 2, 3, ins[0].data_ptr(), eng.nnz_aug, *(t.data_ptr() for t in ins[1:]))
        for entry, tail in (("ce_vjp_qp_many_wave", (dA.data_ptr(), dq.data_ptr(), dP.data_ptr(), adj.data_ptr(), None)),
                            ("ce_vjp_qp_many_params_wave", (2, imap.data_ptr(), imap.data_ptr(), imap.data_ptr(), vmap.data_ptr(), g.data_ptr(), dq.data_ptr(), adj.data_ptr(), None))):
            rc = getattr(L, entry)(*head, *tail)
            torch.cuda.synchronize()
            msg = L.ce_last_error().decode()
            assert rc != 0 and msg.startswith(entry + ":") and why in msg, (rc, msg)
            assert all(bool((t == 7).all()) for t in (dA, dq, dP, g, adj))
    c = case("lp_vertex")
    with pytest.raises(RuntimeError, match="qp_many"):          # with P_bm the wave route is the search-free elimination's alone
        c["eng"].vjp_many(*c["dev"], c["dx"][:1], c["dy"][:1], path="per_instance", P_bm=c["P_bm"], wave=True)
    with pytest.raises(RuntimeError, match="does not serve"):
        big.vjp_many(*ins[:1], *ins[2:5], ins[5], ins[6], path="per_instance", P_bm=ins[1], qp_many=True, wave=True)

"""k_jvp_wave_many (ce_jvp_many_wave): K tangents of a small template, one wave per (instance, chunk of KC), at the planted points of tests/test_gpu_bwd_wave.py
(its SHAPES and case(), its bound 1e-9 = cond 3.3e3 x 2^-53 x 96 x 10: the same points, the same matrix J) against ns_edge_kit's dense solve per tangent, which
accepts every planted instance.  K = 1, KC and KC + 1 of the served row: one lane, a full chunk, and a second wave with one tangent."""
import numpy as np
import pytest
import torch

import ns_edge_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_bwd_wave import B, BOUND, SHAPES, case
from test_gpu_ns_mode_edges import _rel

pytestmark = pytest.mark.gpu

NAMES = ["lp_vertex", "row0_full", "row1_first", "row2_full", "vertex_full", "many_small", "one_cone_full"]
CHUNK = {0: 8, 1: 16, 2: 16}          # KC of the variant list's rows
_MANY: dict = {}


def many(name, duplicate_row=False):
    """KC + 1 seeded Gaussian tangents of a shape on the device, (K, B, .), and the dense answer to each: built once, shared, not changed"""
    key = (name, duplicate_row)
    if key not in _MANY:
        c = case(name, duplicate_row)
        kc = c["eng"].jvp_wave_many_plan()[2]
        ts = [K.tangents(c["pt"], seed=1 + k) for k in range(kc + 1)]
        ev = [c["tpl"].values_from_dense(*t[:3]) for t in ts]
        _MANY[key] = dict(kc=kc, tA=torch.from_numpy(np.stack([a.T for a, _ in ev])).cuda().contiguous(), tq=torch.from_numpy(np.stack([q.T for _, q in ev])).cuda().contiguous(),
                          want=[K.dense_jvp(c["pt"], t) for t in ts])
    return _MANY[key]


def run(c, tA, tq, **kw):
    A, x, y, s = c["dev"][:4]
    out = c["eng"].jvp_many(A, x, y, s, tA, tq, path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"], method="direct", **kw)
    return (*out, c["eng"].last_lsqr_iters)


@pytest.mark.parametrize("which", ["one", "chunk", "chunk_plus_one"])
@pytest.mark.parametrize("name", NAMES)
def test_against_the_dense_solve(name, which):
    c, mc = case(name), many(name)
    eng, kc = c["eng"], mc["kc"]
    variant, lds, chunk = eng.jvp_wave_many_plan()
    assert variant == eng.newton_wave_plan()[0] and chunk == CHUNK[variant] == kc and lds > eng.newton_wave_plan()[1]
    Kt = {"one": 1, "chunk": kc, "chunk_plus_one": kc + 1}[which]
    dx, dy, ds, st, its = run(c, mc["tA"][:Kt], mc["tq"][:Kt], wave=True)
    assert eng.last_jvp_kernel == "ce_jvp_many_wave" and eng.last_jvp_many_path == "many" and dx.shape == (Kt, B, eng.n)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and (its.cpu().numpy() == 0).all()
    for k in range(Kt):
        want = mc["want"][k]
        assert want[3].all()
        e = np.max([_rel(g[k].cpu().numpy(), w) for g, w in zip((dx, dy, ds), want[:3])], axis=0)
        print(f"{name} K={Kt} k={k}: forward derivative max {e.max():.3e} (bound {BOUND:.0e})")
        assert e.max() < BOUND, (k, e)


def test_a_tangent_depends_on_neither_its_lane_nor_its_chunk_nor_the_instances_position():
    c, mc = case("row1_full"), many("row1_full")
    kc = mc["kc"]
    tA, tq = (torch.cat([t[:kc], t[:1]]).contiguous() for t in (mc["tA"], mc["tq"]))          # tangent 0 again, alone in the second chunk
    tA[3] = 0; tq[3] = 0                                                                       # and an all-zero tangent among them
    base = run(c, tA, tq, wave=True)
    assert all(torch.equal(o[0], o[kc]) for o in base) and all((o[3] == 0).all() for o in base)
    shifted = run(c, tA[1:].contiguous(), tq[1:].contiguous(), wave=True)          # every tangent one lane lower
    assert all(torch.equal(o, b[1:]) for o, b in zip(shifted, base))
    nul = run(c, None, tq[:2].contiguous(), wave=True), run(c, torch.zeros_like(tA[:2]), tq[:2].contiguous(), wave=True)          # a null tA is a zero tA
    assert all(torch.equal(a, b) for a, b in zip(*nul))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(B)).cuda()
    inv = torch.argsort(perm)
    cp = dict(c, dev=[t[perm].contiguous() for t in c["dev"]], q=c["q"][:, perm].contiguous())
    got = run(cp, tA[:, perm].contiguous(), tq[:, perm].contiguous(), wave=True)
    assert all(torch.equal(o[:, inv], b) for o, b in zip(got, base))
    sA, sq = tA[:, 0].contiguous(), tq[:, 0].contiguous()          # one (K, .) tangent for the whole batch (batch stride 0) against its expansion
    shared = run(c, sA, sq, wave=True)
    full = run(c, sA[:, None].expand(-1, B, -1).contiguous(), sq[:, None].expand(-1, B, -1).contiguous(), wave=True)
    assert all(torch.equal(a, b) for a, b in zip(shared, full)) and not (shared[0] == 0).all()


def test_transpose_identity_with_the_many_cotangent_wave_adjoint():
    c, mc = case("row1_full"), many("row1_full")
    Kt = mc["kc"] + 1
    rng = np.random.default_rng(43)
    xb, yb = (torch.from_numpy(rng.standard_normal((Kt, B, d))).cuda() for d in (c["n"], c["eng"].m))
    dx, dy, _, st, _ = run(c, mc["tA"], mc["tq"], wave=True)
    A, x, y, s = c["dev"][:4]
    dA, dq, adj = c["eng"].vjp_many(A, x, y, s, xb, yb, path="per_instance", lsqr=TIGHT_LSQR, q_eval=c["q"], wave=True)
    # <xb_j, dx_k> + <yb_j, dy_k> = <dA_j, tA_k> + <dq_j, tq_k> for every pair (j, k) and instance
    lhs = (torch.einsum("jbi,kbi->jkb", xb, dx) + torch.einsum("jbi,kbi->jkb", yb, dy)).cpu().numpy()
    rhs = (torch.einsum("jbi,kbi->jkb", dA, mc["tA"]) + torch.einsum("jbi,kbi->jkb", dq, mc["tq"])).cpu().numpy()
    ti = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
    print(f"K x K transpose identity max {ti.max():.3e} (bound 1e-6)")
    assert (st.cpu().numpy() == 0).all() and (adj.cpu().numpy() == 0).all() and (ti < 1e-6).all() and np.abs(lhs).max() > 1e-3, ti.max()


def test_a_redundant_equality_row_is_flagged_once_and_resolved_for_every_tangent():
    c, mc = case("row1_full", duplicate_row=True), many("row1_full", duplicate_row=True)
    odd = np.arange(B) % 2 == 1
    odd_t = torch.from_numpy(odd).cuda()
    got = run(c, mc["tA"], mc["tq"], wave=True)          # KC + 1 tangents: two waves flag each odd instance
    ref = run(c, mc["tA"], mc["tq"])
    assert c["eng"].last_jvp_kernel == "ce_jvp_many"
    torch.cuda.synchronize()
    assert (got[3].cpu().numpy() == np.where(odd, 12, 0)[None, :]).all(), got[3]
    for g, r in zip(got, ref):          # the same LSQR launch re-solves them: the same bits
        assert torch.equal(g[:, odd_t], r[:, odd_t])
    for k in range(mc["kc"] + 1):          # (the dense solve leaves the singular odd instances out: they are LSQR's above)
        want = mc["want"][k]
        e = np.max([_rel(g[k].cpu().numpy()[~odd], w[~odd]) for g, w in zip(got[:3], want[:3])], axis=0)
        assert want[3][~odd].all() and e.max() < BOUND, (k, e)


def test_refusals_leave_the_outputs_untouched():
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    c, L = case("row1_full"), _lib.lib()
    tpl = P.dense_template(4, dict(z=0, l=3, q=[], ep=1, p=[]))
    exp_eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))
    assert exp_eng.jvp_wave_many_plan() == (-1, 0, 0)
    f64 = dict(dtype=torch.float64, device="cuda")
    Kt = 3
    for eng, q, why in ((exp_eng, c["q"], "exponential"), (c["eng"], None, "q_vals == NULL")):
        z = torch.zeros((Kt, 2, eng.nnz_aug + eng.n + eng.m), **f64)
        out, iout = torch.full((Kt, 2, eng.nnz_aug + eng.m), 7.0, **f64), torch.full((Kt, 2), 7, dtype=torch.int32, device="cuda")
        q_args = (q.data_ptr(), 2, 1) if q is not None else (None, 0, 0)
        p, o, io = z.data_ptr(), out.data_ptr(), iout.data_ptr()
        rc = L.ce_jvp_many_wave(eng._h, 2, Kt, p, eng.nnz_aug, *q_args, p, p, p, p, 2 * eng.nnz_aug, eng.nnz_aug, None, 0, 0, o, o, o, io, io, 1e-8, 1e-8, 1e8, 0, None)
        torch.cuda.synchronize()
        msg = L.ce_last_error().decode()
        assert rc == -2 and "ce_jvp_many_wave:" in msg and why in msg and "use ce_jvp_many" in msg, (rc, msg)
        assert (out == 7).all() and (iout == 7).all()
    with pytest.raises(NotImplementedError, match="ce_jvp_many_wave"):
        exp_eng.jvp_many(*(torch.zeros((2, k), **f64) for k in (exp_eng.nnz_aug, exp_eng.n, exp_eng.m, exp_eng.m)), None, torch.zeros((Kt, 2, exp_eng.n + 1), **f64),
                         path="per_instance", q_eval=torch.zeros((exp_eng.n + 1, 2), **f64), method="direct", wave=True)

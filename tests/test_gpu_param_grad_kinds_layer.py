"""solver_args {"param_grad": "factors", <the kind's many-cotangent key>} through CvxpyLayer.jacobian(direction="reverse") on small hand-built layers with
exponential cones, a PSD block, a PSD block beside exponential cones, and a native quadratic objective -- against the same call under the many-cotangent key alone
(the dA route of the same kernel on the same solve, which is deterministic).

Every parameter entry of the cone layers and of the one-triangle QP layer has exactly ONE entry in the transposed parameter maps (asserted), so the bound of
tests/test_gpu_param_grad_kinds.py -- equality on a row with one map entry -- asks for torch.equal of every Jacobian block.  The full-structure QP layer maps
parameter P[i, j] to structure entry (i, j) and the plugin symmetrises the values: its P block has the symmetrisation's two entries, 1/2 dP[(i, j)] and
1/2 dP[(j, i)], and the bound t 2^-52 sum |val entry| with t = 2 is 2^-52 (|a| + |b|) >= 2^-51 |(a + b) / 2|: asserted in that smaller form, 2^-51 |reference|."""
import dataclasses
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import kit
import psd_tri_ns_kit as PTK
import tri_ns_kit as TK
from cvxpylayers_amd import problems as P
from cvxpylayers_amd.interfaces.param_grad import compose_maps
from cvxpylayers_amd.interfaces.solver_args import _WARNED
from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
from cvxpylayers_amd.torch.templates import template_from_affine_builder
from test_gpu_param_grad_layer import KEY, _loss_grads, layer_of, params_of

pytestmark = pytest.mark.gpu

ARGS = {"eps": 1e-9, "max_iters": 200000}
B = 4
NQ = 5
_L: dict = {}
# kind -> (the many-cotangent key, the dA route's entry, the factor route's entry)
ROUTE = {"exp": ({"tri_adjoint": "search_free"}, "ce_vjp_tri_many", "ce_vjp_tri_many_params"),
         "psd": ({"psd_adjoint": "search_free"}, "ce_vjp_psd_many", "ce_vjp_psd_many_params"),
         "logdet": ({"psd_adjoint": "search_free"}, "ce_vjp_psd_tri_many", "ce_vjp_psd_tri_many_params"),
         "qp": ({"qp_adjoint": "search_free"}, "ce_vjp_qp_many", "ce_vjp_qp_many_params"),
         "qp_full": ({"qp_adjoint": "search_free"}, "ce_vjp_qp_many", "ce_vjp_qp_many_params")}


def _qp_builder(bp, qp, Pp):
    n = NQ
    A = np.zeros((1 + n, n)); A[0] = 1.0; A[1:] = -np.eye(n)          # sum x = b_0, x >= -b_1..n
    return A, bp, qp, 0.5 * (Pp + Pp.T)


def setup(kind):
    """(layer, parameters): built once, shared, not changed"""
    if kind in _L:
        return _L[kind]
    if kind in ("exp", "logdet"):
        kt, name = (TK, "exp_small") if kind == "exp" else (PTK, "logdet_like")
        n, cones = kt.SHAPES[name][0], kt.SHAPES[name][1]
        m = P.cone_rows(cones)
        A, b, c = P.generate(n, cones, B, seed=kt.SHAPES[name][3])
        tpl = template_from_affine_builder(lambda Ap, bp, cp: (Ap, bp, cp), [(m, n), (m,), (n,)], {"s": [], **cones}, [VariableRecovery(slice(0, n), None, (n,))])
        params = tuple(torch.from_numpy(t).cuda() for t in (A, b, c))
    elif kind == "psd":
        k = 3; d = k * (k + 1) // 2
        tpl = template_from_affine_builder(lambda Cm: kit.sdp_min_eig(0.5 * (Cm + Cm.T))[:3], [(k, k)], {"z": 1, "l": 0, "q": [], "s": [k]}, [VariableRecovery(slice(0, d), None, (d,))])
        params = (torch.from_numpy(np.random.default_rng(4).standard_normal((B, k, k))).cuda(),)
    else:
        n = NQ
        tpl = template_from_affine_builder(_qp_builder, [(1 + n,), (n,), (n, n)], {"z": 1, "l": n, "q": [], "s": []}, [VariableRecovery(slice(0, n), None, (n,))])
        if kind == "qp_full":          # the same layer on a full structure: parameter P[i, j] (Fortran order: i + j n) IS structure entry (i, j); the plugin symmetrises the values
            off = tpl.col_offsets[2]
            Pmap = sp.csr_array((np.ones(n * n), (np.arange(n * n), off + np.arange(n * n))), shape=(n * n, tpl.n_params_total + 1))
            tpl = dataclasses.replace(tpl, P_map=Pmap, P_structure=(np.tile(np.arange(n), n).astype(np.int32), (np.arange(n + 1) * n).astype(np.int32), (n, n)))
        torch.manual_seed(3)
        G = torch.randn(B, n, n, dtype=torch.float64, device="cuda")
        bt = torch.cat([torch.ones(B, 1, dtype=torch.float64, device="cuda"), 0.05 * torch.rand(B, n, dtype=torch.float64, device="cuda")], dim=1)
        params = (bt, 0.1 * torch.randn(B, n, dtype=torch.float64, device="cuda"), G @ G.transpose(1, 2) / n + torch.eye(n, dtype=torch.float64, device="cuda"))
    layer = CvxpyLayer(template=tpl, solver_args=ARGS)
    terms = np.diff(layer._A.matT.indptr)[:-1] + np.diff(layer._q.matT.indptr)[:-1] + (np.diff(layer._P.matT.indptr)[:-1] if layer._P is not None else 0)
    assert (terms == 1).all(), (kind, terms)          # one map entry per parameter entry: the derived bound is equality (qp_full: before the symmetrisation's two)
    _L[kind] = (layer, params)
    return _L[kind]


@pytest.mark.parametrize("kind", list(ROUTE))
def test_reverse_jacobian_under_both_keys_equals_the_many_key_alone(kind):
    layer, ps = setup(kind)
    many, entry_d, entry = ROUTE[kind]
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert eng.param_grad_variant == -1
    n_out = int(layer._rec["primal"][0].mat.shape[0])
    per_cot = B * ((eng.m + 1 + eng.n) + (eng.n + 1)) * 8          # what the factor route allocates per cotangent: records and dq; no dP
    small = n_out * per_cot
    several = small // (B * (eng.nnz_aug + eng.nnz_p) * 8) < n_out          # the dA route needs several chunks for them
    assert several or kind == "psd", (small, eng.nnz_aug)          # (the one-block SDP's rows are sparser than its records: ten values against twenty-one)
    outs_d, jac_d = layer.jacobian(*ps, max_bytes=small, solver_args=many)
    info_d = layer.info
    assert info_d["adjoint"]["path"] == entry_d and "param_grad" not in info_d["adjoint"] and (info_d["adjoint"]["status"].shape[0] < n_out) == several
    _, jac_full = layer.jacobian(*ps, solver_args=many)
    st_d = layer.info["adjoint"]["status"]
    calls = []
    orig = eng.vjp_many_params
    eng.vjp_many_params = lambda *a, **k: (calls.append(int(a[4].shape[0])), orig(*a, **k))[1]
    try:
        outs, jac = layer.jacobian(*ps, max_bytes=small, solver_args={**KEY, **many})
        info = layer.info
        assert calls == [n_out], calls
        assert info["adjoint"]["path"] == entry and info["adjoint"]["param_grad"] == "factors" and eng.last_vjp_many_path == "many_params" and eng.last_vjp_kernel == entry
        assert tuple(info["adjoint"]["status"].shape) == (n_out, B) and torch.equal(info["adjoint"]["status"], st_d)
        calls.clear()
        _, jac_1 = layer.jacobian(*ps, max_bytes=1, solver_args={**KEY, **many})          # one cotangent per chunk
        assert calls == [1] * n_out, calls
    finally:
        eng.vjp_many_params = orig
    assert torch.equal(outs[0], outs_d[0])
    for j in range(len(ps)):
        assert jac[0][j].shape == jac_d[0][j].shape and jac[0][j].dtype == torch.float64
        assert torch.equal(jac_d[0][j], jac_full[0][j])
        assert torch.equal(jac_1[0][j], jac[0][j]), (kind, j, "a result depends on the chunk it travelled in")
        err = float((jac[0][j] - jac_d[0][j]).abs().max())
        print(f"{kind} jac[0][{j}]: max |factors - dA route| = {err:.3e}, max |reference| = {float(jac_d[0][j].abs().max()):.3e}")
        if kind == "qp_full" and j == 2:
            assert ((jac[0][j] - jac_d[0][j]).abs() <= 2.0 ** -51 * jac_d[0][j].abs()).all(), (kind, j, err)
        else:
            assert torch.equal(jac[0][j], jac_d[0][j]), (kind, j, err)
    assert sum(float(jac[0][j].abs().max()) for j in range(len(ps))) > 1e-3          # (not vacuous)


def test_the_full_structure_map_carries_the_symmetrisations_two_entries():
    layer, _ = setup("qp_full")
    cm = layer._pg_maps()
    quad = layer.ctx.solver_ctx.quad
    assert not quad.one_triangle and cm.nnz_p == NQ * NQ
    off = layer.template.col_offsets[2]
    isP = (cm.code < 0) & ((cm.code & (1 << 30)) != 0)
    for i in range(NQ):
        for j in range(NQ):
            r = off + i + j * NQ
            t = np.arange(cm.ptr[r], cm.ptr[r + 1])
            assert isP[t].all()
            if i == j:
                assert cm.kidx[t].tolist() == [i + j * NQ] and cm.val[t].tolist() == [1.0]
            else:
                assert sorted(cm.kidx[t].tolist()) == sorted([i + j * NQ, j + i * NQ]) and cm.val[t].tolist() == [0.5, 0.5]
    tri, _ = setup("qp")
    cmt = tri._pg_maps()
    offt = tri.template.col_offsets[2]
    assert tri.ctx.solver_ctx.quad.one_triangle
    assert all(cmt.val[cmt.ptr[offt + i + j * NQ]] == (0.5 if i == j else 1.0) * (1.0 if i != j else 2.0) for i in range(NQ) for j in range(NQ))          # 1/2 of the builder, doubled off the diagonal


def test_raise_on_error_false_with_one_infeasible_instance_keeps_its_nan_pattern():
    layer, (bt, qt, Pt) = setup("qp")
    bt = bt.clone(); bt[2, 0] = -1.0; bt[2, 1:] = 0.0          # sum x = -1 with x >= 0: instance 2 is infeasible
    many = ROUTE["qp"][0]
    args = {"raise_on_error": False, **many}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, jac_d = layer.jacobian(bt, qt, Pt, solver_args=args)
        _, jac = layer.jacobian(bt, qt, Pt, solver_args={**args, **KEY})
    assert int(layer.info["status"][2]) < 0 and layer.info["adjoint"]["param_grad"] == "factors" and layer.info["adjoint"]["path"] == "ce_vjp_qp_many_params"
    for j in range(3):
        assert torch.isnan(jac[0][j][2]).all() and torch.equal(torch.isnan(jac[0][j]), torch.isnan(jac_d[0][j]))
        assert torch.equal(torch.nan_to_num(jac[0][j]), torch.nan_to_num(jac_d[0][j]))


@pytest.mark.parametrize("kind", ["exp", "qp"])
def test_backward_and_forward_ad_under_both_keys_give_one_notice_and_the_defaults_bits(kind):
    import torch.autograd.forward_ad as fwAD
    layer, ps = setup(kind)
    many = ROUTE[kind][0]
    need = [True] * len(ps)
    outs_d, grads_d, info_d = _loss_grads(layer, ps, need, solver_args=many)
    _WARNED.discard("param_grad_unserved")
    with pytest.warns(UserWarning, match="param_grad='factors' is not served for one cotangent") as rec:
        outs, grads, info = _loss_grads(layer, ps, need, solver_args={**KEY, **many})
        _loss_grads(layer, ps, need, solver_args={**KEY, **many})
    assert sum("param_grad" in str(w.message) for w in rec) == 1
    assert "param_grad" not in info["adjoint"] and info["adjoint"]["path"] == info_d["adjoint"]["path"] and set(info) == set(info_d)
    assert torch.equal(outs[0], outs_d[0]) and all(torch.equal(g, gd) for g, gd in zip(grads, grads_d))
    _WARNED.discard("param_grad_unserved")
    fwd = {**many, **({"jvp_mode": "direct"} if kind == "qp" else {})}          # (a quadratic objective inside the kernels has the direct forward derivative alone)
    with fwAD.dual_level():
        duals = [fwAD.make_dual(p, torch.ones_like(p)) for p in ps]
        with pytest.warns(UserWarning, match="forward-mode AD"):
            out = layer(*duals, solver_args={**KEY, **fwd})
        t = fwAD.unpack_dual(out[0]).tangent
        t_d = fwAD.unpack_dual(layer(*duals, solver_args=fwd)[0]).tangent
        assert t is not None and torch.equal(t, t_d)


def test_without_the_many_key_the_layers_keep_the_default_route_with_the_notice():
    layer, ps = setup("exp")
    _, jac_d = layer.jacobian(*ps)
    _WARNED.discard("param_grad_unserved")
    with pytest.warns(UserWarning, match="param_grad='factors' is not served"):
        _, jac = layer.jacobian(*ps, solver_args=KEY)
    assert "param_grad" not in layer.info["adjoint"] and all(torch.equal(a, b) for a, b in zip(jac[0], jac_d[0]))


@pytest.mark.parametrize("kind", ["Abc", "bc"])
def test_the_layers_own_map_has_an_empty_constant_row_and_the_plain_kind_keeps_its_bits(kind):
    """the plain-kind layers of test_gpu_param_grad_layer.py: the composed map is the full composition with the constant column's row dropped, and Jacobians and
    .backward() gradients under the key equal the default route's"""
    layer = layer_of(kind)
    ps = params_of(kind)
    cm = layer._pg_maps()
    tpl = layer.template
    full = compose_maps(layer._A.matT, layer._q.matT, tpl.A_structure[0], tpl.A_structure[1], cm.n, cm.m)
    assert full[0][-1] > full[0][-2], "the layer has constant entries: the full map's last row is not empty"
    assert cm.rows == tpl.n_params_total + 1 and cm.ptr[-1] == cm.ptr[-2] == full[0][-2]
    assert np.array_equal(cm.ptr[:-1], full[0][:-1]) and all(np.array_equal(a, f[:cm.ptr[-1]]) for a, f in zip((cm.code, cm.kidx, cm.val), full[1:]))
    outs_d, jac_d = layer.jacobian(*ps)
    outs, jac = layer.jacobian(*ps, solver_args=KEY)
    assert layer.info["adjoint"]["param_grad"] == "factors"
    for i in range(2):
        for j in range(len(ps)):
            assert torch.equal(jac[i][j], jac_d[i][j]), (kind, i, j)
    need = [True] * len(ps)
    _, grads_d, _ = _loss_grads(layer, ps, need)
    _, grads, info = _loss_grads(layer, ps, need, solver_args=KEY)
    assert info["adjoint"]["param_grad"] == "factors" and all(torch.equal(g, gd) for g, gd in zip(grads, grads_d))

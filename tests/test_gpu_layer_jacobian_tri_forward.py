"""CvxpyLayer.jacobian in the FORWARD direction on a layer with exponential / power cones, under solver_args tri_tangents="many": one ce_jvp_tri_many call per chunk
(each instance factored once, its triples diagonalised once, one LSQR launch for the flagged instances of every tangent) instead of the loop of ce_jvp calls.

The layer is test_gpu_layer_jacobian_tri.py's: min c^T x s.t. A x + s = b, s in K with the cones of tri_ns_kit's exp_pow_mixed (n = 12, m = 24), parameters A (24, 12),
b (24,), c (12,), B = 8 instances of problems.generate.  The forward Jacobian under the key agrees with the default forward loop and with the reverse Jacobian within
1e-6 relative (the bound of test_gpu_layer_jacobian_forward.py and test_gpu_layer_jacobian_tri.py) on the instances no route flags; flags, iteration counts and the
re-solved instances' columns are the loop's bit for bit; info["jvp"] names the kernel; chunking is bit-equal to one chunk; the default call is today's; forward-mode
AD with one tangent ignores the key."""
import numpy as np
import pytest
import torch

import tri_ns_kit as K
from cvxpylayers_amd import problems as P
from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
from cvxpylayers_amd.torch.templates import template_from_affine_builder

pytestmark = pytest.mark.gpu

B = 8
MANY = {"tri_tangents": "many"}
_CACHE: dict = {}


def _setup():
    """the layer, its parameters and the three Jacobians every test compares: computed once, shared, not changed"""
    if _CACHE:
        return _CACHE
    n, cones, _, seed, _ = K.SHAPES["exp_pow_mixed"]
    m = P.cone_rows(cones)
    A, b, c = P.generate(n, cones, B, seed=seed)
    tpl = template_from_affine_builder(lambda Ap, bp, cp: (Ap, bp, cp), [(m, n), (m,), (n,)], {**cones, "s": []}, [VariableRecovery(slice(0, n), None, (n,))])
    layer = CvxpyLayer(template=tpl, solver_args={"eps": 1e-10, "max_iters": 200000})
    params = tuple(torch.from_numpy(t).cuda() for t in (A, b, c))
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    outs_r, jac_r = layer.jacobian(*params, direction="reverse")
    rev = (outs_r, jac_r, dict(layer.info["adjoint"]))
    outs_l, jac_l = layer.jacobian(*params, direction="forward")
    loop = (outs_l, jac_l, eng.last_jvp_many_path, eng.last_jvp_kernel, dict(layer.info["jvp"]))
    outs_m, jac_m = layer.jacobian(*params, direction="forward", solver_args=MANY)
    many = (outs_m, jac_m, eng.last_jvp_many_path, eng.last_jvp_kernel, dict(layer.info["jvp"]))
    _CACHE.update(layer=layer, eng=eng, params=params, n=n, m=m, rev=rev, loop=loop, many=many)
    return _CACHE


def test_the_forward_jacobian_under_the_key_runs_many_and_agrees_with_the_loop_and_the_reverse_jacobian():
    """fails on a tree without the mode: tri_tangents is not a known solver argument there, and the call under it runs the loop"""
    c = _setup()
    n, m = c["n"], c["m"]
    outs_r, jac_r, info_r = c["rev"]
    outs_l, jac_l, path_l, kernel_l, info_l = c["loop"]
    outs_m, jac_m, path_m, kernel_m, info_m = c["many"]
    assert path_l == "loop" and kernel_l == "ce_jvp" and info_l["path"] == "direct" and info_l["kernel"] == "ce_jvp"
    assert path_m == "many" and kernel_m == "ce_jvp_tri_many" and info_m["path"] == "direct" and info_m["kernel"] == "ce_jvp_tri_many"
    Kp = m * n + m + n
    assert info_m["status"].shape == info_l["status"].shape == (Kp, B) and info_m["iters"].shape == (Kp, B)
    assert torch.equal(info_m["status"], info_l["status"]) and torch.equal(info_m["iters"], info_l["iters"])          # the same rule flags, the same solves re-solve
    st_m, st_r = info_m["status"].cpu().numpy(), info_r["status"].cpu().numpy()
    reg = (st_m == 0).all(axis=0)
    both = reg & (st_r == 0).all(axis=0)
    print("status under the key", np.bincount(st_m.ravel()).tolist(), "reverse", np.bincount(st_r.ravel()).tolist(), "instances unflagged by all", int(both.sum()), "of", B)
    assert both.mean() >= 0.5, (st_m, st_r)
    assert torch.equal(outs_m[0], outs_l[0]) and torch.equal(outs_m[0], outs_r[0])
    assert jac_m[0][0].shape == (B, n, m, n) and jac_m[0][1].shape == (B, n, m) and jac_m[0][2].shape == (B, n, n)
    sel, fl = torch.from_numpy(both).cuda(), torch.from_numpy(~reg).cuda()
    assert float(jac_r[0][1][sel].abs().max()) > 1e-3
    for j in range(3):
        for want, what in ((jac_l[0][j], "the forward loop"), (jac_r[0][j], "the reverse Jacobian")):
            e = float((jac_m[0][j][sel] - want[sel]).abs().max() / (1 + want[sel].abs().max()))
            print(f"jac[0][{j}] under the key against {what}: {e:.2e}")
            assert e < 1e-6, (j, what, e)
        assert torch.equal(jac_m[0][j][fl], jac_l[0][j][fl]), j          # a flagged instance's columns: the same LSQR solves


def test_several_chunks_give_the_one_chunk_result():
    c = _setup()
    layer, eng, n, m = c["layer"], c["eng"], c["n"], c["m"]
    calls = []
    orig = eng.jvp_many
    eng.jvp_many = lambda *a, **kw: (calls.append(int(next(t for t in a[4:6] if t is not None).shape[0])), orig(*a, **kw))[1]
    try:
        _, jac_c = layer.jacobian(*c["params"], direction="forward", solver_args=MANY, max_bytes=100 * B * (n + m) * 8)
    finally:
        del eng.jvp_many
    assert len(calls) > 1 and sum(calls) == m * n + m + n and eng.last_jvp_kernel == "ce_jvp_tri_many", calls
    for j in range(3):
        assert torch.equal(jac_c[0][j], c["many"][1][0][j]), j


def test_the_default_and_the_loop_value_are_bit_identical_and_a_third_value_is_refused():
    c = _setup()
    layer, eng = c["layer"], c["eng"]
    _, jac_p = layer.jacobian(*c["params"], direction="forward", solver_args={"tri_tangents": "loop"})
    assert eng.last_jvp_many_path == "loop" and eng.last_jvp_kernel == "ce_jvp" and layer.info["jvp"]["kernel"] == "ce_jvp"
    for j in range(3):
        assert torch.equal(jac_p[0][j], c["loop"][1][0][j]), j
    with pytest.raises(ValueError, match="tri_tangents"):
        layer.jacobian(*c["params"], direction="forward", solver_args={"tri_tangents": "one"})
    # the reverse direction and "auto" (here: more parameter entries than outputs -> reverse) do not read the key
    for direction in ("reverse", "auto"):
        _, jac_a = layer.jacobian(*c["params"], direction=direction, solver_args=MANY)
        for j in range(3):
            assert torch.equal(jac_a[0][j], c["rev"][1][0][j]), (direction, j)


def test_forward_mode_ad_with_one_tangent_ignores_the_key():
    import torch.autograd.forward_ad as fwAD
    c = _setup()
    layer, eng = c["layer"], c["eng"]
    gen = torch.Generator(device="cpu").manual_seed(3)
    tans = [torch.randn(p.shape, dtype=p.dtype, generator=gen).cuda() for p in c["params"]]
    got = []
    for args in ({"jvp_mode": "direct"}, {"jvp_mode": "direct", **MANY}):
        with fwAD.dual_level():
            duals = [fwAD.make_dual(p, t) for p, t in zip(c["params"], tans)]
            eng.last_jvp_many_path = "untouched"
            (x,) = layer(*duals, solver_args=args)
            got.append(fwAD.unpack_dual(x).tangent)
            assert eng.last_jvp_many_path == "untouched" and eng.last_jvp_kernel == "ce_jvp"
    assert got[0] is not None and torch.equal(got[0], got[1])

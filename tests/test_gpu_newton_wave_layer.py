"""solver_args newton_kernel="wave" through CvxpyLayer: the Newton steps of refine_steps and newton_first and the direct forward derivative by k_newton_wave (one
instance per wave) against the default route of the same layer on the same inputs.  Served layer of tests/test_gpu_fwd_wave_layer.py (n = 16, z 2, l 10, q [4, 16],
parameters A, b, c, B = 16).  Without the key info has no "kernel" entry; the entropy layer (one exponential cone) ignores the key with one notice."""
import warnings

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from cvxpylayers_amd.interfaces.solver_args import _WARNED
from test_gpu_fwd_wave_layer import B, exp_layer, params, run, served_layer

pytestmark = pytest.mark.gpu

KEY = {"newton_kernel": "wave"}
LOOSE = {"eps": 1e-4, "refine_steps": 2}


def test_refinement_and_newton_first_under_the_key():
    layer, ps = served_layer(), params()
    tight = run(layer, ps, solver_args={"eps": 1e-11, "max_iters": 200000})[0]
    base = run(layer, ps, solver_args=LOOSE)
    got = run(layer, ps, solver_args={**LOOSE, **KEY})
    assert "kernel" not in base[2]["refine"] and base[2]["refine"]["path"] == "ns"
    assert got[2]["refine"]["kernel"] == "k_newton_wave" and got[2]["refine"]["path"] == "ns"
    r_got, r_base = (i["refine"]["resid_after"].cpu().numpy() for i in (got[2], base[2]))
    d_got, d_base = (max(np.abs(o - t).max() for o, t in zip(r[0], tight)) for r in (got, base))
    print(f"rho after two steps: wave {r_got.max():.3e} workgroup {r_base.max():.3e}; distance to the eps 1e-11 point: wave {d_got:.3e} workgroup {d_base:.3e}")
    assert r_got.max() <= r_base.max(), (r_got.max(), r_base.max())
    assert d_got <= 10 * d_base, (d_got, d_base)
    run(layer, ps, solver_args={"eps": 1e-4})          # a point to warm-start from
    nf = run(layer, ps, solver_args={"eps": 1e-8, "newton_first": 2, **KEY}, warm_start=True)
    assert nf[2]["newton_first"]["refine"]["kernel"] == "k_newton_wave", nf[2]["newton_first"]
    again = run(layer, ps, solver_args=LOOSE)          # the key leaves nothing behind: the default route gives its bits again
    assert "kernel" not in again[2]["refine"]
    for a_, b_ in zip(again[0] + again[1], base[0] + base[1]):
        assert np.array_equal(a_, b_)


def test_forward_mode_under_the_key():
    layer, ps = served_layer(), params()
    tans = [torch.from_numpy(np.random.default_rng(11 + k).standard_normal(tuple(p.shape))).cuda() for k, p in enumerate(ps)]
    out = {}
    for name, args in (("base", {"jvp_mode": "direct"}), ("wave", {"jvp_mode": "direct", **KEY})):
        with fwAD.dual_level():
            duals = [fwAD.make_dual(p.detach(), t) for p, t in zip(ps, tans)]
            res = layer(*duals, solver_args=args)
            out[name] = [fwAD.unpack_dual(o).tangent.cpu().numpy() for o in res], dict(layer.info["jvp"])
    assert out["base"][1]["kernel"] == "ce_jvp" and out["wave"][1]["kernel"] == "ce_jvp_wave" and out["wave"][1]["path"] == "direct"
    for g, g0 in zip(out["wave"][0], out["base"][0]):
        rel = np.abs(g - g0).max() / (1 + np.abs(g0).max())
        print(f"tangent {g.shape}: {rel:.3e} (bound 1e-9)")
        assert rel < 1e-9, rel


def test_unserved_layer_ignores_the_key_with_one_notice():
    layer = exp_layer()
    g = torch.linspace(0.4, 0.9, B, dtype=torch.float64).reshape(B, 1).cuda().requires_grad_(True)
    base = run(layer, (g,), solver_args={"refine_steps": 1})
    _WARNED.discard("newton_kernel_none")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = run(layer, (g,), solver_args={"refine_steps": 1, **KEY})
        got2 = run(layer, (g,), solver_args={"refine_steps": 1, **KEY})
    assert len([w for w in rec if "newton_kernel" in str(w.message)]) == 1, [str(w.message) for w in rec]
    assert "kernel" not in got[2]["refine"] and layer.ctx.solver_ctx.engine(torch.device("cuda", 0)).newton_wave_plan() == (-1, 0)
    for a_, b_ in zip(got[0] + got[1] + got2[0] + got2[1], (base[0] + base[1]) * 2):
        assert np.array_equal(a_, b_)

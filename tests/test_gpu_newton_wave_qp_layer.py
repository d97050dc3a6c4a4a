"""solver_args newton_kernel="wave" on a QP node through CvxpyLayer: the Newton steps of refine_steps and the direct forward derivative of the box / simplex
projection of tests/test_gpu_bwd_wave_qp_layer.py (P = I, n = 12, B = 16, that file's inputs) by k_newton_wave_qp against the default route of the same layer on
the same inputs.  Two refinement steps behind an eps 1e-4 solve: the kernel's name in info, a residual no larger than the default route's and a distance to the
eps 1e-11 point within ten times its; forward-mode AD within 1e-9 relative of ce_jvp_qp's tangents (tests/test_gpu_newton_wave_layer.py's bounds for the same
comparisons); a following call without the key has no such entry and gives the default route's bits."""
import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from test_gpu_bwd_wave_qp_layer import inputs
from test_gpu_fwd_wave_layer import run
from test_gpu_fwd_wave_qp_layer import projection_layer

pytestmark = pytest.mark.gpu

KEY = {"newton_kernel": "wave"}
LOOSE = {"eps": 1e-4, "refine_steps": 2}


def test_refinement_under_the_key_against_the_default_route():
    layer, ps = projection_layer(), inputs()
    tight = run(layer, ps, solver_args={"eps": 1e-11, "max_iters": 200000})[0]
    base = run(layer, ps, solver_args=LOOSE)
    got = run(layer, ps, solver_args={**LOOSE, **KEY})
    assert layer.ctx.solver_ctx.engine(torch.device("cuda", 0)).newton_wave_qp_plan()[0] >= 0
    assert "kernel" not in base[2]["refine"] and base[2]["refine"]["path"] == "ns"
    assert got[2]["refine"]["kernel"] == "k_newton_wave_qp" and got[2]["refine"]["path"] == "ns"
    r_got, r_base = (i["refine"]["resid_after"].cpu().numpy() for i in (got[2], base[2]))
    d_got, d_base = (max(np.abs(o - t).max() for o, t in zip(r[0], tight)) for r in (got, base))
    print(f"rho after two steps: wave {r_got.max():.3e} workgroup {r_base.max():.3e}; distance to the eps 1e-11 point: wave {d_got:.3e} workgroup {d_base:.3e}")
    assert r_got.max() <= r_base.max(), (r_got.max(), r_base.max())
    assert d_got <= 10 * d_base, (d_got, d_base)
    run(layer, ps, solver_args={"eps": 1e-4})          # a point to warm-start from
    nf = run(layer, ps, solver_args={"eps": 1e-8, "newton_first": 2, **KEY}, warm_start=True)
    assert nf[2]["newton_first"]["refine"]["kernel"] == "k_newton_wave_qp", nf[2]["newton_first"]
    again = run(layer, ps, solver_args=LOOSE)          # the key leaves nothing behind: the default route gives its bits again
    assert "kernel" not in again[2]["refine"]
    for a_, b_ in zip(again[0] + again[1], base[0] + base[1]):
        assert np.array_equal(a_, b_)


def test_forward_mode_under_the_key():
    layer, ps = projection_layer(), inputs()
    tans = [torch.from_numpy(np.random.default_rng(11 + k).standard_normal(tuple(p.shape))).cuda() for k, p in enumerate(ps)]
    out = {}
    for name, args in (("base", {"jvp_mode": "direct"}), ("wave", {"jvp_mode": "direct", **KEY})):
        with fwAD.dual_level():
            duals = [fwAD.make_dual(p.detach(), t) for p, t in zip(ps, tans)]
            res = layer(*duals, solver_args=args)
            out[name] = [fwAD.unpack_dual(o).tangent.cpu().numpy() for o in res], dict(layer.info["jvp"])
    assert out["base"][1]["kernel"] == "ce_jvp_qp" and out["wave"][1]["kernel"] == "ce_jvp_qp_wave" and out["wave"][1]["path"] == "direct"
    assert (out["wave"][1]["status"].cpu().numpy() == 0).all()
    for g, g0 in zip(out["wave"][0], out["base"][0]):
        rel = np.abs(g - g0).max() / (1 + np.abs(g0).max())
        print(f"tangent {g.shape}: {rel:.3e} (bound 1e-9)")
        assert rel < 1e-9 and np.abs(g0).max() > 1e-3, rel

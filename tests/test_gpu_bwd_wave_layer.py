"""solver_args adjoint_kernel="wave" through CvxpyLayer: the backward pass by k_bwd_wave (one instance per wave) against the default route of the same layer on the
same inputs.  Served layer of tests/test_gpu_fwd_wave_layer.py (n = 16, z 2, l 10, q [4, 16], parameters A, b, c, eps 1e-8, B = 16): parameter gradients within
1e-5 relative (that file's bound) alone, beside forward_kernel="wave", under param_grad="factors" and under raise_on_error=False; info["adjoint"]["kernel"] names
the kernel; a following call without the key has no such entry and gives the default route's bits.  The entropy layer (one exponential cone) ignores the key with
one notice."""
import warnings

import numpy as np
import pytest
import torch

from cvxpylayers_amd.interfaces.solver_args import _WARNED
from test_gpu_fwd_wave_layer import B, exp_layer, params, run, served_layer

pytestmark = pytest.mark.gpu

KEY = {"adjoint_kernel": "wave"}


@pytest.mark.parametrize("extra", [{}, {"forward_kernel": "wave"}, {"param_grad": "factors"}, {"raise_on_error": False}], ids=["alone", "both_keys", "factors", "no_raise"])
def test_backward_under_the_key_against_the_default_route(extra):
    layer, ps = served_layer(), params()
    base = run(layer, ps)
    assert "kernel" not in base[2]["adjoint"]          # without the key: no such entry
    got = run(layer, ps, solver_args={**KEY, **extra})
    assert got[2]["adjoint"]["kernel"] == "k_bwd_wave"
    if "forward_kernel" in extra:          # a whole step on wave kernels
        assert got[2]["forward"] == {"kernel": "k_fwd_wave"}
    assert (got[2]["adjoint"]["status"].cpu().numpy() == 0).all()
    for g, g0 in zip(got[1], base[1]):
        rel = np.abs(g - g0).max() / (1 + np.abs(g0).max())
        print(f"{extra} gradient {g.shape}: {rel:.3e} (bound 1e-5)")
        assert rel < 1e-5, rel
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert eng.bwd_wave_plan()[0] >= 0 and eng.last_adjoint_kernel == "k_bwd_wave"
    again = run(layer, ps)
    assert "kernel" not in again[2]["adjoint"] and eng.last_adjoint_kernel is None
    for a_, b_ in zip(again[0] + again[1], base[0] + base[1]):          # the key leaves nothing behind
        assert np.array_equal(a_, b_)


def test_unserved_layer_ignores_the_key_with_one_notice():
    layer = exp_layer()
    g = torch.linspace(0.4, 0.9, B, dtype=torch.float64).reshape(B, 1).cuda().requires_grad_(True)
    base = run(layer, (g,))
    _WARNED.discard("adjoint_kernel_none")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = run(layer, (g,), solver_args=KEY)
        got2 = run(layer, (g,), solver_args=KEY)
    assert len([w for w in rec if "adjoint_kernel" in str(w.message)]) == 1, [str(w.message) for w in rec]
    assert got[2]["adjoint"]["kernel"] == "workgroup" == got2[2]["adjoint"]["kernel"]
    assert layer.ctx.solver_ctx.engine(torch.device("cuda", 0)).bwd_wave_plan() == (-1, 0)
    for a_, b_ in zip(got[0] + got[1] + got2[0] + got2[1], (base[0] + base[1]) * 2):
        assert np.array_equal(a_, b_)

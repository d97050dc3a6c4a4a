"""solver_args adjoint_kernel="wave" on a QP node through CvxpyLayer: the backward pass of the box / simplex projection of tests/test_gpu_fwd_wave_qp_layer.py (P = I,
n = 12, eps 1e-8, B = 16, that file's inputs) by k_bwd_wave_qp against the default route of the same layer on the same inputs.  The forward outputs are bit-equal
(the key does not touch the solve), info["adjoint"]["kernel"] names the kernel, every adjoint status is 0 and the parameter gradients are within 1e-5 relative -- the
bound of test_gpu_bwd_wave_layer.py for the same comparison; beside forward_kernel="wave" both wave kernels are reported.  A following call without the key has no
such entry and gives the default route's bits; layer.jacobian under the key reports the path it reports without it."""
import numpy as np
import pytest
import torch

from test_gpu_fwd_wave_layer import run
from test_gpu_fwd_wave_qp_layer import B, N, projection_layer

pytestmark = pytest.mark.gpu

KEY = {"adjoint_kernel": "wave"}


def inputs():
    rng = np.random.default_rng(2)
    return tuple(torch.from_numpy(t).cuda().requires_grad_(True) for t in (rng.standard_normal((B, N)), -0.05 * rng.random((B, N)), 0.1 + 0.2 * rng.random((B, N))))


@pytest.mark.parametrize("extra", [{}, {"forward_kernel": "wave"}], ids=["alone", "both_keys"])
def test_qp_backward_under_the_key_against_the_default_route(extra):
    layer, ps = projection_layer(), inputs()
    base = run(layer, ps)
    assert "kernel" not in base[2]["adjoint"]          # without the key: no such entry
    got = run(layer, ps, solver_args={**KEY, **extra})
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert got[2]["adjoint"]["kernel"] == "k_bwd_wave_qp" and eng.bwd_wave_qp_plan()[0] >= 0 and eng.last_adjoint_kernel == "k_bwd_wave_qp"
    if extra:          # a whole step on wave kernels
        assert got[2]["forward"] == {"kernel": "k_fwd_wave_qp"}
    else:
        assert "forward" not in got[2] and all(np.array_equal(a_, b_) for a_, b_ in zip(got[0], base[0]))
    assert (got[2]["adjoint"]["status"].cpu().numpy() == 0).all()
    for g, g0 in zip(got[1], base[1]):
        rel = np.abs(g - g0).max() / (1 + np.abs(g0).max())
        print(f"{extra} gradient {g.shape}: {rel:.3e} (bound 1e-5)")
        assert rel < 1e-5, rel
    again = run(layer, ps)
    assert "kernel" not in again[2]["adjoint"] and eng.last_adjoint_kernel is None
    for a_, b_ in zip(again[0] + again[1], base[0] + base[1]):          # the key leaves nothing behind
        assert np.array_equal(a_, b_)


def test_jacobian_keeps_its_path_under_the_key():
    layer, ps = projection_layer(), inputs()
    layer.jacobian(*ps)
    path = layer.info["adjoint"]["path"]
    layer.jacobian(*ps, solver_args=KEY)
    assert layer.info["adjoint"]["path"] == path

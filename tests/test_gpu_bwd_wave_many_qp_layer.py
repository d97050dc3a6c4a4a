"""layer.jacobian(direction="reverse") of a QP node under solver_args {"qp_adjoint": "search_free", "adjoint_kernel": "wave"}: the many-cotangent calls run
k_bwd_wave_many_qp (ce_vjp_qp_many_wave) and agree with the same Jacobian under qp_adjoint="search_free" alone (ce_vjp_qp_many) within 1e-5 relative -- the layer
tests' bound for this comparison (tests/test_gpu_bwd_wave_qp_layer.py) -- with every status 0; a following call without the wave key reports ce_vjp_qp_many and gives
the earlier bits.  The projection layer and inputs of tests/test_gpu_fwd_wave_qp_layer.py / test_gpu_bwd_wave_qp_layer.py."""
import numpy as np
import pytest
import torch

from test_gpu_bwd_wave_qp_layer import inputs
from test_gpu_fwd_wave_qp_layer import projection_layer

pytestmark = pytest.mark.gpu

FREE = {"qp_adjoint": "search_free"}


def jac(layer, ps, **sa):
    _outs, J = layer.jacobian(*[p.detach() for p in ps], solver_args=sa, direction="reverse")
    torch.cuda.synchronize()
    return [j.cpu().numpy() for row in J for j in row], layer.info["adjoint"]


def test_reverse_jacobian_under_both_keys_runs_the_wave_kernel():
    layer, ps = projection_layer(), inputs()
    base, info0 = jac(layer, ps, **FREE)
    assert info0["path"] == "ce_vjp_qp_many"
    got, info = jac(layer, ps, **FREE, adjoint_kernel="wave")
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert info["path"] == "ce_vjp_qp_many_wave" and eng.last_adjoint_kernel == "k_bwd_wave_many_qp" and eng.bwd_wave_many_qp_plan()[0] >= 0
    assert (info["status"].cpu().numpy() == 0).all() and (info0["status"].cpu().numpy() == 0).all()
    for j, j0 in zip(got, base):
        rel = np.abs(j - j0).max() / (1 + np.abs(j0).max())
        print(f"Jacobian block {j.shape}: {rel:.3e} (bound 1e-5)")
        assert rel < 1e-5, rel
    again, info1 = jac(layer, ps, **FREE)
    assert info1["path"] == "ce_vjp_qp_many" and eng.last_adjoint_kernel is None
    assert all(np.array_equal(a_, b_) for a_, b_ in zip(again, base))          # the key leaves nothing behind

"""layer.jacobian(direction="reverse") under solver_args adjoint_kernel="wave": every many-cotangent call of the Jacobian runs k_bwd_wave_many (ce_vjp_many_wave, under
param_grad="factors" ce_vjp_many_params_wave) and agrees with the same call without the key within tests/test_gpu_bwd_wave.py's 1e-9; without the key
info["adjoint"]["path"] is what it was; a layer the kernel does not serve ignores the key.  Layers of tests/test_gpu_fwd_wave_layer.py."""
import numpy as np
import pytest
import torch

from test_gpu_bwd_wave import BOUND
from test_gpu_fwd_wave_layer import B, exp_layer, params, served_layer

pytestmark = pytest.mark.gpu

KEY = {"adjoint_kernel": "wave"}


def jac(layer, ps, **sa):
    outs, J = layer.jacobian(*[p.detach() for p in ps], solver_args=sa, direction="reverse")
    torch.cuda.synchronize()
    return [j.cpu().numpy() for row in J for j in row], layer.info


@pytest.mark.parametrize("extra, entry", [({}, "ce_vjp_many_wave"), ({"param_grad": "factors"}, "ce_vjp_many_params_wave")], ids=["dA", "factors"])
def test_reverse_jacobian_under_the_key_against_the_default_route(extra, entry):
    layer, ps = served_layer(), params()
    base, info0 = jac(layer, ps, **extra)
    path0 = info0["adjoint"]["path"]
    assert path0 == ("ce_vjp_many_params" if extra else "per_instance") and "kernel" not in info0["adjoint"]
    got, info = jac(layer, ps, **KEY, **extra)
    assert info["adjoint"]["path"] == entry and info["adjoint"]["kernel"] == "k_bwd_wave"
    assert (info["adjoint"]["status"].cpu().numpy() == 0).all()
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert eng.last_adjoint_kernel == "k_bwd_wave_many" and eng.bwd_wave_many_plan()[0] == 1
    for j, j0 in zip(got, base):
        rel = np.abs(j - j0).reshape(B, -1).max(axis=1) / (1 + np.abs(j0).reshape(B, -1).max(axis=1))
        print(f"{entry} block {j.shape}: {rel.max():.3e} (bound {BOUND:.0e})")
        assert rel.max() < BOUND, rel.max()
    again, info1 = jac(layer, ps, **extra)          # the key leaves nothing behind
    assert info1["adjoint"]["path"] == path0 and eng.last_adjoint_kernel is None
    assert all(np.array_equal(a, b) for a, b in zip(again, base))


def test_unserved_layer_ignores_the_key():
    layer = exp_layer()
    g = torch.linspace(0.4, 0.9, B, dtype=torch.float64).reshape(B, 1).cuda()
    base, info0 = jac(layer, (g,))
    got, info = jac(layer, (g,), **KEY)
    assert info["adjoint"]["path"] == info0["adjoint"]["path"] and info["adjoint"]["kernel"] == "workgroup"
    assert layer.ctx.solver_ctx.engine(torch.device("cuda", 0)).bwd_wave_many_plan() == (-1, 0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(got, base))

"""layer.jacobian(direction="forward") under solver_args newton_kernel="wave": every many-tangent call of the Jacobian runs k_jvp_wave_many (ce_jvp_many_wave) and
agrees with the same call without the key within tests/test_gpu_bwd_wave.py's 1e-9; without the key info["jvp"] is what it was; a layer the kernel does not serve
ignores the key.  Layers of tests/test_gpu_fwd_wave_layer.py."""
import numpy as np
import pytest
import torch

from test_gpu_bwd_wave import BOUND
from test_gpu_fwd_wave_layer import B, exp_layer, params, served_layer

pytestmark = pytest.mark.gpu

KEY = {"newton_kernel": "wave"}


def jac(layer, ps, **sa):
    outs, J = layer.jacobian(*[p.detach() for p in ps], solver_args=sa, direction="forward")
    torch.cuda.synchronize()
    return [j.cpu().numpy() for row in J for j in row], layer.info


def test_forward_jacobian_under_the_key_against_the_default_route():
    layer, ps = served_layer(), params()
    base, info0 = jac(layer, ps)
    assert info0["jvp"]["kernel"] == "ce_jvp_many" and info0["jvp"]["path"] == "direct"
    got, info = jac(layer, ps, **KEY)
    assert info["jvp"]["kernel"] == "ce_jvp_many_wave" and info["jvp"]["path"] == "direct"
    assert (info["jvp"]["status"].cpu().numpy() == 0).all() and (info["jvp"]["iters"].cpu().numpy() == 0).all()
    assert layer.ctx.solver_ctx.engine(torch.device("cuda", 0)).jvp_wave_many_plan()[0] == 1
    for j, j0 in zip(got, base):
        rel = np.abs(j - j0).reshape(B, -1).max(axis=1) / (1 + np.abs(j0).reshape(B, -1).max(axis=1))
        print(f"block {j.shape}: {rel.max():.3e} (bound {BOUND:.0e})")
        assert rel.max() < BOUND, rel.max()
    again, info1 = jac(layer, ps)          # the key leaves nothing behind
    assert info1["jvp"]["kernel"] == "ce_jvp_many"
    assert all(np.array_equal(a, b) for a, b in zip(again, base))


def test_unserved_layer_ignores_the_key():
    layer = exp_layer()
    g = torch.linspace(0.4, 0.9, B, dtype=torch.float64).reshape(B, 1).cuda()
    base, info0 = jac(layer, (g,))
    kernel0 = info0["jvp"]["kernel"]
    got, info = jac(layer, (g,), **KEY)
    assert info["jvp"]["kernel"] == kernel0 != "ce_jvp_many_wave"
    assert layer.ctx.solver_ctx.engine(torch.device("cuda", 0)).jvp_wave_many_plan() == (-1, 0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(got, base))
